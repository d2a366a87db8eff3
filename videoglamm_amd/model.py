"""Drop-in façade for the reference's ``VideoGLaMMForCausalLM`` inference surface
(R/model/VideoGLaMM.py:560-596 inference, :598-768 inference_framewise, :770-879 inference_video_branch,
:325-508 model_forward(inference=True), :897-900 forward) on the MI355X kernel library.

Same argument meaning, return structure and error behaviour as the reference for this path; batch size 1 is
asserted exactly like R/model/VideoGLaMM.py:252-253.
"""
import os

import torch

from . import ops
from .params import Params
from .sam2 import SAM2
from .vlm import VisionTowers, generate, stage_mark


class _Cfg:
    """model.config: the attributes R/chat.py:296-331 reads and assigns (seg_token_idx, eos/bos/pad ids, use_sam2, ...)."""

    def __init__(self, d):
        self.__dict__.update(d)


class _Tower:
    """What get_vision_tower() / get_image_vision_tower() hand to R/chat.py:316-319,335-351: an object whose dtype / device
    movers are no-ops — the towers' weights live in the model's packed parameter store and follow the model."""

    def __init__(self, name):
        self.name, self.is_loaded = name, True

    def to(self, *a, **k):
        return self

    half = bfloat16 = float = cuda = eval = lambda self, *a, **k: self

    def __repr__(self):
        return f"<{self.name} (weights packed inside VideoGLaMMForCausalLM)>"


class _Inner:
    """model.get_model() / model.model: config + the vision-module initialisers of VideoGPTPlusMetaModel
    (R/model/videogpt_plus/model/arch.py:14-85).  The reference builds and loads the towers there; here they arrive with the
    checkpoint (ingest.load_state_dict), so the initialiser only checks that they are present."""

    def __init__(self, outer):
        self._outer = outer
        self.config = outer.config
        self.vision_tower = _Tower("InternVideo2 video tower")
        self.image_vision_tower = _Tower("CLIP image tower")

    def initialize_vision_modules(self, model_args=None, fsdp=None):
        sd = self._outer.P.sd
        for prefix in ("model.vision_tower.vision_encoder.", "model.image_vision_tower.vision_tower."):
            if not any(k.startswith(prefix) for k in sd):
                raise RuntimeError(f"no {prefix}* tensors in the checkpoint: pass vision_tower / image_vision_tower to from_pretrained")

    def get_vision_tower(self):
        return self.vision_tower

    def get_image_vision_tower(self):
        return self.image_vision_tower


class GenerationConfig:
    """model.generation_config: the decoding fields of the checkpoint's generation_config.json this build follows (do_sample, temperature,
    top_k, top_p; HF's defaults when absent) — assignable like model.config.eos_token_id (R/chat.py:305).  The other fields HF would turn into a
    logits processor or warper keep their neutral values unless the checkpoint sets them; a non-neutral one is refused when sampling."""

    def __init__(self, d=None):
        from .ingest import GENERATION_DEFAULTS, GENERATION_UNSUPPORTED
        self.__dict__.update(GENERATION_DEFAULTS)
        self.__dict__.update(GENERATION_UNSUPPORTED)
        self.__dict__.update(d or {})

    def __repr__(self):
        return f"GenerationConfig({self.__dict__})"


def resolve_sampling(gc, do_sample=None, temperature=None, top_k=None, top_p=None, generator=None):
    """precedence keyword > model.generation_config (which starts as the checkpoint's) -> None (greedy) or vlm.generate's dict(T, k, p, seed).
    The seed is one draw from `generator` (torch's default CPU generator when None), taken only when sampling: torch.manual_seed(n)
    reproduces a run, and greedy runs leave the RNG alone."""
    from .ingest import GENERATION_UNSUPPORTED
    pick = lambda v, name: getattr(gc, name) if v is None else v
    if not pick(do_sample, "do_sample"):
        return None
    for name, neutral in GENERATION_UNSUPPORTED.items():
        v = getattr(gc, name, neutral)
        if v is not None and v != neutral and not (name == "no_repeat_ngram_size" and int(v) <= 0):
            raise NotImplementedError(f"generation_config.{name} = {v!r}: this build samples with temperature / top_k / top_p only")
    T, k, p = pick(temperature, "temperature"), pick(top_k, "top_k"), pick(top_p, "top_p")
    T = 1.0 if T is None else float(T)
    k = 0 if k is None else int(k)
    p = 1.0 if p is None else float(p)
    if not T > 0:      # TemperatureLogitsWarper
        raise ValueError(f"`temperature` (={T}) has to be a strictly positive float, otherwise your next token scores will be invalid.")
    if k < 0:          # TopKLogitsWarper
        raise ValueError(f"`top_k` has to be a strictly positive integer, but is {k}")
    if p < 0 or p > 1.0:     # TopPLogitsWarper
        raise ValueError(f"`top_p` has to be a float > 0 and < 1, but is {p}")
    seed = int(torch.empty((), dtype=torch.int64).random_(generator=generator))
    return dict(T=T, k=k, p=p, seed=seed)


class VideoGLaMMForCausalLM:
    def __init__(self, state_dict, config, torch_dtype=torch.bfloat16, device="cuda", use_sam2_video_branch=False,
                 comm=None, **kwargs):
        """state_dict: the merged checkpoint ({name: tensor}, reference naming); config: dict with keys
        seg_token_idx, iv2{depth,num_heads,patch_size}, clip{num_layers,num_heads,patch_size},
        llm{hidden,num_layers,num_heads,num_kv_heads,rms_eps,rope_theta}, sam2{image_size,trunk{...}},
        optional eos_token_id.  comm: optional videoglamm_amd.dist.FrameSharder for multi-GPU runs."""
        from . import _lib

        _lib.load()  # fail loudly if the HIP extension is missing: there is no fallback path
        self.cfg = dict(config)
        self.config = _Cfg(dict(seg_token_idx=config["seg_token_idx"], use_sam2=True, eos_token_id=config.get("eos_token_id"),
                                bos_token_id=config.get("bos_token_id"), pad_token_id=config.get("pad_token_id"),
                                mm_use_im_start_end=False, mm_use_im_patch_token=False))
        if torch_dtype == torch.float16:
            raise NotImplementedError("the MI355X kernels compute in bfloat16 or float32 (same 16-bit storage as fp16, wider exponent): "
                                      "pass torch_dtype=torch.bfloat16")
        for k in ("load_in_8bit", "load_in_4bit", "quantization_config"):
            if kwargs.get(k):
                raise NotImplementedError(f"{k}: bitsandbytes quantisation (R/chat.py:247-272) is CUDA-only; the fp8 LLM path of this build is "
                                          "cfg['llm']['decode_weights'] = cfg['llm']['prefill_gemm'] = 'fp8', and the native 4-bit (MXFP4) decode "
                                          "weights are cfg['llm']['decode_weights'] = 'mxfp4' (with cfg['llm']['prefill_gemm'] = 'mxfp4' and "
                                          "cfg['llm']['dense_mlp'] = 'drop' the prefill runs on them too and the dense MLP weights are let go)")
        self.dtype = torch_dtype
        self.device = torch.device(device)
        if self.device.type == "cuda":
            # the C-ABI launches go to HIP's CURRENT device and torch's current stream of it (ops._stream): bind this process to the
            # model's device (one process per GPU) instead of launching on device 0 against device-k pointers
            self.device = torch.device("cuda", torch.cuda.current_device() if self.device.index is None else self.device.index)
            torch.cuda.set_device(self.device)
        self.use_sam2_video_branch = use_sam2_video_branch
        # HF generate()'s decoding mode: greedy unless the checkpoint's generation_config.json (or the caller) sets do_sample
        self.generation_config = GenerationConfig(config.get("generation"))
        self._sampling = None
        self._build(state_dict)
        self.model = _Inner(self)
        self.comm = comm
        # > 0: clear 4-connected blobs smaller than this from the thresholded masks ON THE DEVICE, before they cross PCIe —
        # what the reference's evaluation does on the host afterwards (remove_small_blobs(min_size=20),
        # R/eval_gcg_infer.py:20-29,182).  0 = the reference's inference() behaviour.
        self.min_blob_size = int(kwargs.get("min_blob_size", 0))
        # this call's return_boxes (set by the inference surface, read by _binarize / _download); _fused: the (masks, box table) pair
        # of a _binarize that filtered the blobs and reduced the boxes in one chain
        self._want_boxes = False
        self._fused = None
        # this call's return_rle / return_masks (same life cycle): run-length codes as one more return value, and whether the dense masks are downloaded
        self._want_rle = False
        self._want_masks = True
        # diagnostics only: when set to a dict, inference() leaves the fp32 mask logits ("logits", device), the [SEG] embeddings
        # ("emb") and the model's own per-step argmaxes ("argmax") in it (bench.py's self-check, tests)
        self.capture = None
        # optional callable (step, emitted id) -> replacement id | None, applied after the lm_head + argmax of every decode step (vlm.generate):
        # teacher forcing in the parity tests, synth.install_forced_tokens for synthetic-weight runs.  None = plain greedy decoding.
        self.token_hook = None
        # diagnostics only: when set to a list, the stages of inference() append (name, host time) after a device sync
        # (bench.py's per-stage replicated / sharded split; meaningful with VG_HIERA_START=serial)
        self.stages = None

    @classmethod
    def from_pretrained(cls, path, config=None, vision_tower=None, image_vision_tower=None, sam2_checkpoint=None,
                        seg_token_idx=None, lora_dir=None, iv2_origin_num_frames=None, **kwargs):
        """The released artefact layout (R/chat.py:277-319): an HF directory (*.safetensors or pytorch_model*.bin shards +
        config.json) with the LLM, the projectors, text_hidden_fcs and SAM2; the InternVideo2 .pt and the CLIP directory
        the config names under mm_vision_tower / image_mm_vision_tower (or given here); optionally a stand-alone SAM2
        checkpoint.  The architecture config is derived from config.json + tensor shapes (videoglamm_amd/ingest.py) unless
        `config` — or a "videoglamm_amd" section in config.json — gives it explicitly."""
        from . import ingest

        sd, hf = ingest.load_state_dict(path, vision_tower, image_vision_tower, sam2_checkpoint, lora_dir=lora_dir,
                                        iv2_origin_num_frames=iv2_origin_num_frames)
        if config is None:
            config = (hf or {}).get("videoglamm_amd") or ingest.derive_config(sd, hf, seg_token_idx)
        if "generation" not in config:
            config = dict(config, generation=ingest.generation_settings((hf or {}).get("_generation_config")))
        return cls(sd, config, **kwargs)

    def _build(self, sd):
        """(re)create the packed parameter store and the graphs over it for self.device / self.dtype (packing is lazy)."""
        self.P = Params(sd, self.device, self.dtype)
        self.towers = VisionTowers(self.P, self.cfg)
        self.sam2 = SAM2(self.P, "model.visual_model.", self.cfg["sam2"])

    # ------------------------------------------------------------------ start-up surface (R/chat.py:277-350)
    def eval(self):
        return self

    def get_model(self):
        return self.model

    def resize_token_embeddings(self, new_num_tokens=None):
        """HF PreTrainedModel.resize_token_embeddings as R/chat.py:300 uses it after tokenizer.add_tokens("[SEG]"): the input
        embedding and the lm_head grow (or shrink) to new_num_tokens rows.  A released checkpoint already has the [SEG] row, so
        this is the identity there.  New rows are ZERO here (HF draws them from N(0, initializer_range): values no checkpoint
        pins) — a zero lm_head row can never win the argmax, i.e. an untrained token is never emitted."""
        sd = self.P.sd
        rows = sd["model.embed_tokens.weight"].shape[0]
        if new_num_tokens is None or new_num_tokens == rows:
            return self
        for name in ("model.embed_tokens.weight", "lm_head.weight"):
            w = sd[name]
            if new_num_tokens < rows:
                sd[name] = w[:new_num_tokens].contiguous()
            else:
                sd[name] = torch.cat([w, torch.zeros(new_num_tokens - w.shape[0], w.shape[1], dtype=w.dtype, device=w.device)])
        self.cfg["llm"] = dict(self.cfg["llm"], vocab=int(new_num_tokens))
        self._build(sd)
        return self

    def _cast(self, dtype=None, device=None):
        dtype = self.dtype if dtype is None else dtype
        device = self.device if device is None else torch.device(device)
        if dtype == torch.float16:
            raise NotImplementedError("float16 is not a compute type of this build: use .bfloat16() or .float()")
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if (dtype, device) != (self.dtype, self.device):
            if self.P.dropped:
                raise RuntimeError("this model dropped its dense MLP weights (cfg['llm']['dense_mlp'] = 'drop'): the state dict no longer holds the "
                                   f"tensors a copy in {dtype} on {device} would be built from; cast or move the model before its first inference, "
                                   "or load the checkpoint again")
            self.dtype, self.device = dtype, device
            if device.type == "cuda":
                torch.cuda.set_device(device)
            self._build(self.P.sd)
        return self

    def bfloat16(self):
        return self._cast(dtype=torch.bfloat16)

    def float(self):
        return self._cast(dtype=torch.float32)

    def half(self):
        return self._cast(dtype=torch.float16)

    def cuda(self, device=None):
        return self._cast(device="cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))

    def to(self, *args, **kwargs):
        dtype, device = kwargs.get("dtype"), kwargs.get("device")
        for a in args:
            if isinstance(a, torch.dtype):
                dtype = a
            else:
                device = f"cuda:{a}" if isinstance(a, int) else a
        return self._cast(dtype, device)

    def _live_cfg(self):
        """the architecture config with the ids the caller may have (re)assigned on model.config (R/chat.py:303-307)."""
        c = self.cfg
        seg = getattr(self.config, "seg_token_idx", c["seg_token_idx"])
        return c if seg == c["seg_token_idx"] else dict(c, seg_token_idx=seg)

    def _eos(self):
        """ids generation stops on, with HF generate()'s precedence (transformers 4.41 GenerationMixin._prepare_generation_config): a
        generation_config.json that names eos ids wins; without one the generation config is derived from model.config, so ids the
        caller assigned on model.config.eos_token_id after load (R/chat.py:305-307) REPLACE the checkpoint's config.json ids."""
        from .ingest import eos_ids
        live = getattr(self.config, "eos_token_id", None)
        if self.cfg.get("eos_from_generation_config") or live is None:
            return eos_ids(self.cfg.get("eos_token_id")) or None
        return eos_ids(live) or None

    # ------------------------------------------------------------------ forward surface
    def forward(self, **kwargs):
        """R/model/VideoGLaMM.py:897-900: LM forward when past_key_values is passed (not part of this path),
        otherwise model_forward."""
        if "past_key_values" in kwargs:
            raise NotImplementedError("the bare LM forward is outside the accelerated path (SURVEY §8)")
        return self.model_forward(**kwargs)

    __call__ = forward

    def model_forward(self, images_for_sam, images, context_images, input_ids, labels=None, attention_masks=None,
                      offset=None, masks_list=None, label_list=None, resize_list=None, inference=False, **kwargs):
        """inference=True branch of R/model/VideoGLaMM.py:325-508: teacher-forced ids -> [SEG] rows -> framewise
        decode; returns {"pred_masks": B x T x [N,H,W] logits, "gt_masks": masks_list}."""
        if not inference:
            raise NotImplementedError("training losses are out of scope (SURVEY §2 rows 10-11)")
        assert len(images) == 1 and input_ids.shape[0] == 1  # batch size is 1 (VideoGLaMM.py:252-253)
        hw = tuple(label_list[0].shape[-2:])
        ids = input_ids[0].cpu()
        _, emb = generate(self.P, self._live_cfg(), self.towers, images[0].to(self.device), context_images[0].to(self.device), ids, 0)
        if emb.shape[0] == 0:
            return {"pred_masks": [[torch.zeros(0, *hw, device=self.device) for _ in range(len(images_for_sam[0]))]], "gt_masks": masks_list}
        logits, _ = self.sam2.framewise_branch(images_for_sam[0].to(self.device), emb, hw)
        return {"pred_masks": [[logits[t] for t in range(logits.shape[0])]], "gt_masks": masks_list}

    def validate(self, samples, ignore_index=255):
        """The validator's loop (R/utils/trainer.py:409-473) over `samples`, an iterable of the keyword dictionaries model_forward takes
        (masks_list = [ground truth [N, T, H, W] of 0 / 1 / ignore_index]): per sample model_forward(inference=True), the class counts of all
        its frames from ONE launch on the logits where they are (postproc.validation_record), and the validator's meters on the host.
        Returns (giou, ciou).  One GPU only."""
        if self.comm is not None:
            raise NotImplementedError("validate() runs on one GPU: the frames of a multi-GPU model are sharded over the ranks; "
                                      "call model_forward() and postproc.validation_record on one GPU")
        from . import postproc

        meter = postproc.ValidationMeter()
        for kw in samples:
            meter.update(postproc.validation_record(self.model_forward(**dict(kw, inference=True)), ignore_index))
        return meter.result()

    # ------------------------------------------------------------------ inference surface
    def inference(self, images, context_images, images_for_sam, input_ids, resize_list, original_size_list,
                  max_new_tokens=32, use_sam2_video_branch=False, *, return_boxes=False, return_rle=False, return_masks=True, return_scores=False,
                  **sampling):
        """R/model/VideoGLaMM.py:560-596.  Keyword-only extras: do_sample / temperature / top_k / top_p (override model.generation_config for
        this call), generator (the torch.Generator the sampling seed is drawn from) and return_boxes: a third return value
        [{frame: {obj: np.float32[4]}}] with the keys of the masks' dictionaries, the postproc.masks_to_boxes value (x_min, y_min, x_max, y_max;
        [1e8, 1e8, 0, 0] for an empty mask) of exactly the mask that is returned, reduced on the device before the masks are downloaded.
        return_rle: one more return value after that, [{frame: {obj: {"size": [H, W], "counts": [int, ...]}}}], COCO's uncompressed run-length code
        (postproc.mask_to_rle_pytorch's form) of the same masks, encoded on the device by one ops.mask_rle call for the whole clip.
        return_masks=False (needs return_boxes or return_rle): the dense masks are not downloaded; the mask dictionaries keep their keys and hold None.
        return_scores: one more return value, last: [{"logprob": float32 [G], "margin": float32 [G], "top2": int64 [G, 2]}] (host numpy, one
        record per generated token): log_softmax of the raw fp32 logits at the token the model picked, the margin between the two largest logits
        and their indices (vg_token_scores_rows inside the decode step).  One GPU only."""
        if self.device.type == "cuda" and torch.cuda.current_device() != self.device.index:
            torch.cuda.set_device(self.device)
        if use_sam2_video_branch:
            if self.config.use_sam2:
                return self.inference_video_branch(images, context_images, images_for_sam, input_ids, resize_list,
                                                   original_size_list, max_new_tokens, return_boxes=return_boxes, return_rle=return_rle,
                                                   return_masks=return_masks, return_scores=return_scores, **sampling)
            raise ValueError("use_sam2_video_branch is True, but model is not configured to use SAM2")
        return self.inference_framewise(images, context_images, images_for_sam, input_ids, resize_list,
                                        original_size_list, max_new_tokens, return_boxes=return_boxes, return_rle=return_rle,
                                        return_masks=return_masks, return_scores=return_scores, **sampling)

    def _set_returns(self, return_boxes, return_rle=False, return_masks=True, return_scores=False):
        """this call's return_boxes / return_rle / return_masks / return_scores; refusals come first, before any GPU work"""
        if return_scores and self.comm is not None:
            raise NotImplementedError("return_scores runs on one GPU: the replicated decode of a multi-GPU model would produce the scores on "
                                      "every rank; call the model on one GPU for them")
        self._want_scores, self._scores = bool(return_scores), None
        if not return_masks and not (return_boxes or return_rle):
            raise ValueError("return_masks=False needs return_boxes=True or return_rle=True: the call would return nothing about the masks")
        if return_boxes and self.comm is not None:
            raise NotImplementedError("return_boxes runs on one GPU: the masks of a multi-GPU model are sharded over the ranks; "
                                      "use postproc.masks_to_boxes on the returned masks")
        if (return_rle or not return_masks) and self.comm is not None:
            raise NotImplementedError("return_rle / return_masks=False run on one GPU: the masks of a multi-GPU model are sharded over the ranks; "
                                      "use postproc.mask_to_rle_pytorch on the returned masks")
        self._want_boxes, self._fused = bool(return_boxes), None
        self._want_rle, self._want_masks = bool(return_rle), bool(return_masks)

    def _returns(self):
        """the three keywords of this call, to hand on to a nested call"""
        return dict(return_boxes=self._want_boxes, return_rle=self._want_rle, return_masks=self._want_masks, return_scores=self._want_scores)

    def _resolve_sampling(self, do_sample=None, temperature=None, top_k=None, top_p=None, generator=None):
        """this call's decoding mode; multi-GPU: every rank adopts rank 0's seed (the decode is replicated and must emit the same ids)"""
        s = resolve_sampling(self.generation_config, do_sample, temperature, top_k, top_p, generator)
        if s is not None and self.comm is not None and self.comm.world > 1:
            s["seed"] = self.comm.broadcast_seed(s["seed"])
        self._sampling = s

    def _text_side(self, images, context_images, input_ids, max_new_tokens, after_prefill=None):
        assert len(images) == 1 and input_ids.shape[0] == 1  # batch size is 1 (VideoGLaMM.py:252-253)
        # context_images=None: single-image prompt (CLIP -> image_mm_projector without pooling, arch.py:243-245,393-397)
        ctx = context_images[0] if context_images is not None else None
        trace = self.capture
        if self._want_scores:      # the records come back through generate()'s trace (a private one when nothing is being captured)
            trace = {} if trace is None else trace
            trace["scores"] = True
        out_ids, emb = generate(self.P, self._live_cfg(), self.towers, images[0].to(self.device), None if ctx is None else ctx.to(self.device),
                                input_ids[0].cpu(), max_new_tokens, self._eos(),
                                token_hook=self.token_hook, after_prefill=after_prefill, comm=self.comm,
                                trace=trace, stages=self.stages, sampling=self._sampling)
        if self._want_scores:
            self._scores = trace["scores"]
        if self.capture is not None:
            self.capture["emb"] = emb
        return out_ids.unsqueeze(0), emb

    def _text_and_hiera(self, images, context_images, sam, input_ids, max_new_tokens, all_frames=False, static_feats=False):
        """LLM side + Hiera features of this rank's frames, Hiera on the side stream (see _hiera_async)."""
        frames = self.comm.my_frames(sam.shape[0]) if self.comm is not None else None
        # single-GPU graph-replayed propagation: Hiera writes the clip's features into the replay's own input buffers (SAM2.video_static_feats)
        bufs = self.sam2.video_static_feats(sam.shape[0]) if (static_feats and frames is None and not all_frames) else None
        box = {}

        def start():
            box["feats"], box["join"] = self._hiera_async(sam, frames, all_frames, bufs)

        # Hiera goes to the side stream FIRST: it then shares the chip with the towers / LLM prefill (big-K, MFMA-bound
        # GEMMs that leave HBM idle, where Hiera's small-K GEMMs, norms and window shuffles are bandwidth-hungry) and is
        # mostly done when the HBM-saturated decode loop starts.  Measured r01: 195 ms/clip vs 200.5 when it is enqueued
        # after the prefill (VG_HIERA_START=prefill) and 211 with no overlap at all.
        mode = os.environ.get("VG_HIERA_START", "first")
        if mode == "serial":      # no overlap (per-kernel timing runs: bench.py's instrumented step)
            stage_mark(self.stages, "begin")
            feats = self.comm.hiera_all_frames(self.sam2, sam) if all_frames else self.sam2.hiera_frames(sam, frames, bufs=bufs)
            stage_mark(self.stages, "hiera_fpn")
            out_ids, emb = self._text_side(images, context_images, input_ids, max_new_tokens)
            return out_ids, emb, feats
        if mode == "first":
            start()
            out_ids, emb = self._text_side(images, context_images, input_ids, max_new_tokens)
        else:
            out_ids, emb = self._text_side(images, context_images, input_ids, max_new_tokens, after_prefill=start)
        box["join"]()
        return out_ids, emb, box["feats"]

    def _binarize(self, logits):
        """[T,N,H,W] fp32 logits -> uint8 masks (logit > 0), small blobs removed when min_blob_size is set."""
        masks = ops.threshold(logits)
        if self._want_boxes and self.min_blob_size > 0:      # blob filter and boxes from one union-find (vg_blob_boxes)
            table, masks = ops.mask_boxes(masks, self.min_blob_size, return_mask=True)
            self._fused = (masks, table)
            return masks
        return ops.remove_small_blobs(masks, self.min_blob_size) if self.min_blob_size > 0 else masks

    @staticmethod
    def _segments(mask_u8, frame_ids=None, obj_ids=None):
        """[T,N,H,W] uint8 (0 / 1) on host -> {frame: {obj: bool ndarray [H,W]}} (VideoGLaMM.py:757-766, 869-875); frame_ids / obj_ids:
        the global indices of the rows / columns (multi-GPU shards), default 0..T-1 / 0..N-1."""
        m = mask_u8.numpy().view(bool)       # 0 / 1 bytes ARE numpy bools: no second pass over the clip's masks
        frame_ids = range(m.shape[0]) if frame_ids is None else frame_ids
        obj_ids = range(m.shape[1]) if obj_ids is None else obj_ids
        return {t: {k: m[i, j] for j, k in enumerate(obj_ids)} for i, t in enumerate(frame_ids)}

    def _fast_masks(self):
        """thresholded masks straight from the low-res logits (vg_bilinear_mask) unless something needs the fp32 logits"""
        return self.capture is None and self.min_blob_size == 0

    def _to_host(self, masks):
        """device uint8 masks -> fresh host tensor.  The destination is a new PINNED tensor from torch's caching host allocator
        (a freed block of an earlier clip after the first call): one DMA, no staging copy — pageable D2H of 32 x 1024^2 masks
        costs ~5 ms, a reused staging buffer plus the host-side copy out of it ~3 ms on top of the 1 ms transfer."""
        if masks.device.type != "cuda":
            return masks
        out = torch.empty(masks.shape, dtype=masks.dtype, pin_memory=True)
        out.copy_(masks, non_blocking=True)
        torch.cuda.current_stream(masks.device).synchronize()
        return out

    def _download(self, masks):
        """device uint8 masks [T,N,H,W] -> (host masks, boxes, codes).  boxes: None or, under return_boxes, float32 ndarray [T,N,4], the boxes of
        all T x N masks from ONE ops.mask_boxes call on the device masks, enqueued before the download (16 bytes per mask cross PCIe on top of the
        masks).  codes: None or, under return_rle, the [T][N] run-length codes of the same masks from ONE ops.mask_rle call (its counts and offsets
        are the two downloads).  Under return_masks=False the dense download is skipped and (T, N) stands in for the host masks."""
        if not (self._want_boxes or self._want_rle):
            return self._to_host(masks), None, None
        boxes = codes = None
        fused, self._fused = self._fused, None
        if self._want_boxes:
            from .postproc import boxes_xyxy
            table = fused[1] if fused is not None and fused[0] is masks else ops.mask_boxes(masks)
            boxes = boxes_xyxy(table)
        if self._want_rle:
            counts, offsets = ops.mask_rle(masks)
        host = self._to_host(masks) if self._want_masks else tuple(masks.shape[:2])
        if self._want_boxes:
            boxes = boxes.cpu().numpy()
        if self._want_rle:
            from .postproc import _split_rle
            T, N = masks.shape[:2]
            flat = _split_rle(counts.cpu(), offsets.cpu(), masks.shape[-2:])
            codes = [flat[i * N:(i + 1) * N] for i in range(T)]
        return host, boxes, codes

    def _with_scores(self, ret):
        """an inference()'s return value, with [the scores] as its last element under return_scores"""
        return ret + ([self._scores],) if self._want_scores else ret

    def _extras(self):
        """how many return values follow the masks: the boxes, then the codes"""
        return int(self._want_boxes) + int(self._want_rle)

    @staticmethod
    def _cut(host, boxes, codes, a, n):
        """objects [a, a + n) of a _download triple"""
        return (host[:, a:a + n] if torch.is_tensor(host) else (host[0], n), None if boxes is None else boxes[:, a:a + n],
                None if codes is None else [row[a:a + n] for row in codes])

    def _result(self, host, boxes=None, codes=None):
        """the tail of an inference()'s return value: ([segments],) and, with the same keys, [boxes] under return_boxes and [codes] under
        return_rle, in that order.  host: _download's first value; None = no [SEG]."""
        if host is None:
            return tuple([{}] for _ in range(1 + self._extras()))
        if torch.is_tensor(host):
            segs = self._segments(host)
        else:                       # return_masks=False: the keys, no pixels
            segs = {t: {k: None for k in range(host[1])} for t in range(host[0])}
        out = [[segs]]
        if self._want_boxes:
            out.append([{t: {k: boxes[i, j] for j, k in enumerate(fr)} for i, (t, fr) in enumerate(segs.items())}])
        if self._want_rle:
            out.append([{t: {k: codes[i][j] for j, k in enumerate(fr)} for i, (t, fr) in enumerate(segs.items())}])
        return tuple(out)

    def _hiera_async(self, sam, frames=None, all_frames=False, bufs=None):
        """Hiera + FPN of the SAM frames on a side HIP stream.  It depends only on the pixels, not on the LLM, and it is
        MFMA/LDS-bound while the LLM decode loop is an HBM-bound GEMV chain: the two overlap on the chip.  Returns
        (features per frame, join) — call join() on the consuming stream before reading the features."""
        # all_frames (multi-GPU video branch, r04): the rank's frames go through Hiera in chunks and every finished chunk is all-gathered right away
        # (FrameSharder.hiera_all_frames) — the object ranks' features arrive while the later chunks and the LLM side still run
        run = (lambda: self.comm.hiera_all_frames(self.sam2, sam)) if all_frames else (lambda: self.sam2.hiera_frames(sam, frames, bufs=bufs))
        if self.device.type != "cuda":
            return run(), (lambda: None)
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device)
        main = torch.cuda.current_stream(self.device)
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side):
            feats = run()

        def join():
            torch.cuda.current_stream(self.device).wait_stream(self._side)
            for f in feats.values():
                for t in f:
                    t.record_stream(torch.cuda.current_stream(self.device))
        return feats, join

    def inference_framewise(self, images, context_images, images_for_sam, input_ids, resize_list, original_size_list,
                            max_new_tokens=32, *, do_sample=None, temperature=None, top_k=None, top_p=None, generator=None, empty_ok=False,
                            return_boxes=False, return_rle=False, return_masks=True, return_scores=False):
        """R/model/VideoGLaMM.py:598-768 -> (output_ids [1,L+G], [ {frame: {obj: mask}} ]).  empty_ok: no [SEG] gives [{}] as the video branch
        does, not the reference's exception (inference_prompts' meaning of such a prompt).  return_boxes / return_rle / return_masks / return_scores: see inference()."""
        self._set_returns(return_boxes, return_rle, return_masks, return_scores)
        self._resolve_sampling(do_sample, temperature, top_k, top_p, generator)
        sam = images_for_sam[0].to(self.device)
        out_ids, emb, feats = self._text_and_hiera(images, context_images, sam, input_ids, max_new_tokens)
        if emb.shape[0] == 0 and empty_ok:
            return self._with_scores((out_ids,) + self._result(None))
        if emb.shape[0] == 0:
            # the reference dereferences `.shape` of a tuple here (VideoGLaMM.py:732): same exception type
            raise AttributeError("'tuple' object has no attribute 'shape'")
        hw = tuple(original_size_list[0])
        if self.comm is not None:
            # this rank's frames under their global indices (the whole clip when the sharder gathers the masks)
            masks, fids = self.comm.framewise(self.sam2, sam, emb, hw, frame_feats=feats, binarize=None if self._fast_masks() else self._binarize)
            host = self._to_host(masks)
            stage_mark(self.stages, "mask_decode")
            return out_ids, [self._segments(host, frame_ids=fids)]
        elif self._fast_masks():
            res = self._download(self.sam2.framewise_branch(sam, emb, hw, frame_feats=feats, as_masks=True)[0])
            stage_mark(self.stages, "mask_decode")
        else:
            logits, _ = self.sam2.framewise_branch(sam, emb, hw, frame_feats=feats)
            if self.capture is not None:
                self.capture["logits"] = logits
            res = self._download(self._binarize(logits))
        return self._with_scores((out_ids,) + self._result(*res))

    def inference_video_branch(self, images, context_images, images_for_sam, input_ids, resize_list, original_size_list,
                               max_new_tokens=32, *, do_sample=None, temperature=None, top_k=None, top_p=None, generator=None,
                               return_boxes=False, return_rle=False, return_masks=True, return_scores=False):
        """R/model/VideoGLaMM.py:770-879; empty dict when no [SEG] was emitted (:840-842).  return_boxes / return_rle / return_masks / return_scores: see inference()."""
        self._set_returns(return_boxes, return_rle, return_masks, return_scores)
        self._resolve_sampling(do_sample, temperature, top_k, top_p, generator)
        sam = images_for_sam[0].to(self.device)
        # multi-GPU: frames shard for Hiera only (the propagation is a recurrence over frames) and every rank needs every frame's features:
        # one exchange of the whole clip after the last frame (default), or — FrameSharder(stream_features=True) — streamed chunk by chunk on a
        # communicator of their own while Hiera still runs
        streamed = self.comm is not None and self.comm.stream_features
        graphed = self.comm is None and self.device.type == "cuda" and os.environ.get("VG_VIDEO_GRAPH", "1") == "1"
        out_ids, emb, feats = self._text_and_hiera(images, context_images, sam, input_ids, max_new_tokens, all_frames=streamed, static_feats=graphed)
        if emb.shape[0] == 0:
            return self._with_scores((out_ids,) + self._result(None))
        hw = tuple(original_size_list[0])
        if self.comm is not None:
            # OBJECTS shard for the propagation
            emb = self.comm.sync_seg_embeddings(emb)
            if not streamed:
                feats = self.comm.gather_frame_feats(feats, sam.shape[0], self.sam2)
            stage_mark(self.stages, "feature_all_gather")
            masks, oids = self.comm.video_branch_objects(self.sam2, sam, emb, hw, feats, binarize=None if self._fast_masks() else self._binarize)
            host = self._to_host(masks)
            stage_mark(self.stages, "propagation")
            return out_ids, [self._segments(host, obj_ids=oids)]
        if self.device.type == "cuda" and os.environ.get("VG_VIDEO_GRAPH", "1") == "1":
            # the propagation replayed from a HIP graph (same launches, same results: tests/test_host_sam2.py): the eager loop leaves
            # the GPU idle 16 % of a C2 clip waiting for Python between ~8000 small launches (r02: 378 -> 361 ms); VG_VIDEO_GRAPH=0 = eager
            fast = self._fast_masks()
            out = self.sam2.video_branch_graphed(sam, emb, hw, feats, as_masks=fast)
            if fast:
                res = self._download(out)
                stage_mark(self.stages, "propagation")
                return self._with_scores((out_ids,) + self._result(*res))
            logits = out
        elif self._fast_masks():
            res = self._download(self.sam2.video_branch(sam, emb, hw, frame_feats=feats, as_masks=True))
            stage_mark(self.stages, "propagation")
            return self._with_scores((out_ids,) + self._result(*res))
        else:
            logits = self.sam2.video_branch(sam, emb, hw, frame_feats=feats)
        if self.capture is not None:
            self.capture["logits"] = logits
        return self._with_scores((out_ids,) + self._result(*self._download(self._binarize(logits))))

    # ------------------------------------------------------------------ several prompts about one clip
    def inference_prompts(self, images, context_images, images_for_sam, input_ids_list, resize_list, original_size_list,
                          max_new_tokens=32, use_sam2_video_branch=False, *, do_sample=None, temperature=None, top_k=None, top_p=None,
                          generator=None, shared=None, return_boxes=False, return_rle=False, return_masks=True, return_scores=False):
        """B prompts ([1, L_b] or [L_b] each) about ONE clip -> (output ids [1, L_b + G_b] per prompt, {frame: {obj: mask}} per prompt).
        return_boxes adds a third list, {frame: {obj: np.float32[4]}} per prompt (see inference(); {} where the masks are {}); return_rle one more
        after it, {frame: {obj: code}} per prompt; return_masks=False leaves None in the mask dictionaries (see inference()); return_scores one more
        list, last, the per-token records of every prompt (see inference()), in prompt order.
        Entry b means what inference(..., input_ids=input_ids_list[b]) means; a prompt without a [SEG] gets {} (as the video branch does,
        R/model/VideoGLaMM.py:840-842).  The towers, Hiera and the prefill of the shared prefix (system text + visual block, identical ids in
        every prompt) run once; SAM2 runs once with every prompt's [SEG] embeddings as its objects.  Sampling draws one seed per prompt from
        `generator`, in list order.  More than 16 prompts run in consecutive groups of 16.
        shared picks the route.  True: the shared route just described, for any model (the decode is one batched step per token wherever
        prompts.batched_route allows it — bf16, fp8 and mxfp4 decode weights).  False: one inference() call per prompt, in list order, for any model:
        nothing is shared, and ids and masks equal inference()'s bit for bit (the shared route's masks need not).  None (the default):
        the shared route, except for a model with cfg["llm"]["decode_weights"] = "mxfp4", which keeps the per-prompt calls it has always had."""
        from .prompts import GROUP, check_prompts
        if self.comm is not None and self.comm.world > 1:
            raise NotImplementedError("inference_prompts() runs on one GPU: call inference() per prompt on a multi-GPU model")
        self._set_returns(return_boxes, return_rle, return_masks, return_scores)
        ids_list = [torch.as_tensor(x).cpu().long() for x in input_ids_list]
        if not ids_list:
            raise NotImplementedError("inference_prompts() needs at least one prompt")
        for b, ids in enumerate(ids_list):
            if ids.dim() == 2:
                assert ids.shape[0] == 1, f"input_ids_list[{b}]: one prompt per entry ([1, L] or [L])"
                ids_list[b] = ids = ids[0]
            assert ids.dim() == 1, f"input_ids_list[{b}]: one prompt per entry ([1, L] or [L])"
        assert len(images) == 1  # one clip (VideoGLaMM.py:252-253)
        if use_sam2_video_branch and not self.config.use_sam2:
            raise ValueError("use_sam2_video_branch is True, but model is not configured to use SAM2")
        check_prompts(ids_list)
        if self.device.type == "cuda" and torch.cuda.current_device() != self.device.index:
            torch.cuda.set_device(self.device)
        if shared is None:
            shared = self._live_cfg()["llm"].get("decode_weights") != "mxfp4"
        if not shared:
            return self._prompts_alone(images, context_images, images_for_sam, ids_list, resize_list, original_size_list, max_new_tokens,
                                       use_sam2_video_branch, dict(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p,
                                                                   generator=generator, **self._returns()))
        samplings = [resolve_sampling(self.generation_config, do_sample, temperature, top_k, top_p, generator) for _ in ids_list]
        out_ids, segs, extras = [], [], [[] for _ in range(self._extras() + int(self._want_scores))]
        for g in range(0, len(ids_list), GROUP):
            o, s, ex = self._prompts_group(images, context_images, images_for_sam, ids_list[g:g + GROUP], original_size_list, max_new_tokens,
                                           use_sam2_video_branch, samplings[g:g + GROUP])
            out_ids += o
            segs += s
            for acc, e in zip(extras, ex):
                acc += e
        return (out_ids, segs, *extras)

    def _prompts_alone(self, images, context_images, images_for_sam, ids_list, resize_list, original_size_list, max_new_tokens, video, sampling):
        """inference_prompts() as one inference() per prompt, in list order (each call draws its own sampling seed from the generator); the
        captures of the calls are gathered per prompt as _prompts_group leaves them."""
        out_ids, segs, extras, caps = [], [], [[] for _ in range(self._extras() + int(self._want_scores))], []
        keep = self.capture
        try:
            for ids in ids_list:
                if keep is not None:
                    self.capture = {}
                if video:
                    o, s, *b = self.inference_video_branch(images, context_images, images_for_sam, ids[None], resize_list, original_size_list,
                                                           max_new_tokens, **sampling)
                else:
                    o, s, *b = self.inference_framewise(images, context_images, images_for_sam, ids[None], resize_list, original_size_list,
                                                        max_new_tokens, empty_ok=True, **sampling)
                out_ids.append(o)
                segs.append(s[0])
                for acc, x in zip(extras, b):
                    acc.append(x[0])
                caps.append(self.capture)
        finally:
            self.capture = keep
        if keep is not None:
            for k in ("argmax", "emb", "logits"):
                if any(k in c for c in caps):
                    keep[k] = [c.get(k) for c in caps]
        return (out_ids, segs, *extras)

    def _prompts_group(self, images, context_images, images_for_sam, ids_list, original_size_list, max_new_tokens, video, samplings):
        from .prompts import generate_prompts
        sam = images_for_sam[0].to(self.device)
        graphed = video and self.device.type == "cuda" and os.environ.get("VG_VIDEO_GRAPH", "1") == "1"
        bufs = self.sam2.video_static_feats(sam.shape[0]) if graphed else None
        box = {}

        def start():
            box["feats"], box["join"] = self._hiera_async(sam, bufs=bufs)

        # VG_HIERA_START as in _text_and_hiera: "first" (default) puts Hiera on the side stream before the towers, "prefill" after the prefix's
        # prefill, "serial" runs it alone first (per-stage timing)
        mode = os.environ.get("VG_HIERA_START", "first")
        if mode == "serial":
            stage_mark(self.stages, "begin")
            feats = self.sam2.hiera_frames(sam, bufs=bufs)
            stage_mark(self.stages, "hiera_fpn")
            box["join"] = lambda: None
        elif mode == "first":
            start()
        ctx = context_images[0] if context_images is not None else None
        traces = [{} for _ in ids_list] if self.capture is not None or self._want_scores else None
        if self._want_scores:
            for t in traces:
                t["scores"] = True
        out, emb, counts = generate_prompts(self.P, self._live_cfg(), self.towers, images[0].to(self.device),
                                            None if ctx is None else ctx.to(self.device), ids_list, max_new_tokens, self._eos(),
                                            token_hook=self.token_hook, samplings=samplings, traces=traces,
                                            after_prefix=start if mode not in ("serial", "first") else None, stages=self.stages)
        box["join"]()
        if mode != "serial":
            feats = box["feats"]
        out = [o.unsqueeze(0) for o in out]
        starts = [sum(counts[:b]) for b in range(len(counts))]
        if self.capture is not None:
            self.capture["argmax"] = [t.get("argmax", []) for t in traces]
            self.capture["emb"] = [emb[a:a + n] for a, n in zip(starts, counts)]
        scores = [[t["scores"] for t in traces]] if self._want_scores else []       # the last extra list: one record set per prompt
        if emb.shape[0] == 0:
            return out, [{} for _ in ids_list], [[{} for _ in ids_list] for _ in range(self._extras())] + scores
        hw = tuple(original_size_list[0])
        fast = self._fast_masks()
        if video:
            if graphed:
                res = self.sam2.video_branch_graphed(sam, emb, hw, feats, as_masks=fast)
            else:
                res = self.sam2.video_branch(sam, emb, hw, frame_feats=feats, as_masks=fast)
        else:
            res = self.sam2.framewise_branch(sam, emb, hw, frame_feats=feats, as_masks=fast)[0]
        if not fast:
            if self.capture is not None:
                self.capture["logits"] = [res[:, a:a + n] for a, n in zip(starts, counts)]
            res = self._binarize(res)
        down = self._download(res)
        stage_mark(self.stages, "propagation" if video else "mask_decode")
        # objects [a, a + n) are prompt b's, renumbered from 0; one list per extra return value (boxes, codes) follows the masks
        per = [self._result(*self._cut(*down, a, n)) if n else self._result(None) for a, n in zip(starts, counts)]
        return out, [p[0][0] for p in per], [[p[i][0] for p in per] for i in range(1, 1 + self._extras())] + scores

    # ------------------------------------------------------------------ several clips, one prompt each
    def inference_clips(self, clips, max_new_tokens=32, use_sam2_video_branch=False, *, do_sample=None, temperature=None, top_k=None, top_p=None,
                        generator=None, return_boxes=False, return_rle=False, return_masks=True, return_scores=False):
        """B clips, one prompt each -> a list whose entry b is what inference(*clips[b], max_new_tokens, use_sam2_video_branch, ...) returns
        (with return_boxes: inference()'s third element, [{frame: {obj: np.float32[4]}}], in every clip's tuple; with return_rle its codes after
        that; return_masks=False as in inference(); with return_scores inference()'s [records] as the last element of every clip's tuple):
        (output ids [1, L_b + G_b], [{frame: {obj: mask}}]), the same ids and the same masks pixel for pixel.  clips[b]: the six per-clip arguments
        of inference() (images, context_images, images_for_sam, input_ids, resize_list, original_size_list) as a tuple or a dict.
        Every clip runs its own towers, Hiera and whole-prompt prefill; the clips of a group (up to 16) then decode together, one row per clip in
        one batched step per token, wherever prompts.batched_route allows it (VG_CLIPS_BATCHED=0: one clip after another), and the mask decode runs
        per clip after the group's decode.  A clip's Hiera features are kept until then (8.4 MB per 1024^2 frame in bf16).  Sampling draws one seed
        per clip from `generator`, in list order: torch.manual_seed(n) before this call gives what it gives before the B inference() calls.
        A clip without a [SEG] behaves as in inference(): [{}] on the video branch, the reference's AttributeError on the framewise one."""
        from .clips import as_clip, groups
        if self.comm is not None and self.comm.world > 1:
            raise NotImplementedError("inference_clips() runs on one GPU: call inference() per clip on a multi-GPU model")
        self._set_returns(return_boxes, return_rle, return_masks, return_scores)
        clips = [as_clip(c, b) for b, c in enumerate(clips)]
        if not clips:
            raise NotImplementedError("inference_clips() needs at least one clip")
        if self.capture is not None or self.stages is not None:
            raise NotImplementedError("model.capture / model.stages are diagnostics of inference() and inference_prompts(): unset them for "
                                      "inference_clips(), or call inference() per clip")
        if use_sam2_video_branch and not self.config.use_sam2:
            raise ValueError("use_sam2_video_branch is True, but model is not configured to use SAM2")
        for b, (images, context_images, images_for_sam, input_ids, _, original_size_list) in enumerate(clips):
            if len(images) != 1 or getattr(input_ids, "ndim", 0) != 2 or input_ids.shape[0] != 1:      # batch size is 1 per clip (VideoGLaMM.py:252-253)
                raise ValueError(f"clips[{b}]: one clip per entry (images of length 1, input_ids [1, L]), as inference() takes them")
        if self.device.type == "cuda" and torch.cuda.current_device() != self.device.index:
            torch.cuda.set_device(self.device)
        samplings = [resolve_sampling(self.generation_config, do_sample, temperature, top_k, top_p, generator) for _ in clips]
        out = []
        # generate_clips groups by 16 itself; the groups are cut here as well so that the Hiera features (and SAM frames) held until the mask
        # decode are those of one group, never of the whole list
        for g0, g1 in groups(len(clips)):
            out += self._clips_group(clips[g0:g1], max_new_tokens, use_sam2_video_branch, samplings[g0:g1])
        return out

    def _clips_group(self, clips, max_new_tokens, video, samplings):
        from .clips import generate_clips
        mode = os.environ.get("VG_HIERA_START", "first")
        sams, feats, joins = {}, {}, {}

        def start(b):
            # Hiera + FPN of clip b on the side stream, as _text_and_hiera starts it; its features live in buffers of their own until the clip's
            # mask decode (the video branch's replay buffers, SAM2.video_static_feats, are shared by every clip of a length: they would alias
            # between the clips of a group, so this entry point takes video_branch_graphed's staged-input form)
            sams[b] = clips[b][2][0].to(self.device)
            if mode == "serial":
                feats[b], joins[b] = self.sam2.hiera_frames(sams[b]), (lambda: None)
            else:
                feats[b], joins[b] = self._hiera_async(sams[b])

        text = []
        for images, context_images, _, input_ids, _, _ in clips:
            ctx = context_images[0] if context_images is not None else None
            text.append((images[0].to(self.device), None if ctx is None else ctx.to(self.device), input_ids[0].cpu()))
        first = mode in ("first", "serial")
        traces = [{"scores": True} for _ in clips] if self._want_scores else None
        res = generate_clips(self.P, self._live_cfg(), self.towers, text, max_new_tokens, self._eos(), token_hook=self.token_hook,
                             samplings=samplings, traces=traces, before_clip=start if first else None, after_prefill=None if first else start)
        out = []
        for b, ((out_ids, emb), clip) in enumerate(zip(res, clips)):
            joins[b]()
            tail = ([traces[b]["scores"]],) if self._want_scores else ()
            out.append((out_ids.unsqueeze(0),) + self._clip_masks(sams.pop(b), emb, feats.pop(b), tuple(clip[5][0]), video) + tail)
        return out

    def _clip_masks(self, sam, emb, feats, hw, video):
        """the single-GPU mask decode of inference_video_branch / inference_framewise for one clip (capture unset): _result's tuple"""
        if emb.shape[0] == 0:
            if video:
                return self._result(None)
            # the reference dereferences `.shape` of a tuple here (VideoGLaMM.py:732): same exception type
            raise AttributeError("'tuple' object has no attribute 'shape'")
        fast = self._fast_masks()
        if video:
            if self.device.type == "cuda" and os.environ.get("VG_VIDEO_GRAPH", "1") == "1":
                res = self.sam2.video_branch_graphed(sam, emb, hw, feats, as_masks=fast)
            else:
                res = self.sam2.video_branch(sam, emb, hw, frame_feats=feats, as_masks=fast)
        else:
            res = self.sam2.framewise_branch(sam, emb, hw, frame_feats=feats, as_masks=fast)[0]
        return self._result(*self._download(res if fast else self._binarize(res)))
