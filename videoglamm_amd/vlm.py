"""LLM side of the VideoGLaMM hot path on the MI355X kernel library (rows L1–L6 of SURVEY.md §8a):
InternVideo2 video tower, CLIP ViT image tower, V-L adapters + 2x2 pooling, embedding splice, Llama
decoder with a KV cache, greedy decode with [SEG] hidden capture, L-V adapter.

Scheduling differs from the reference on purpose (results are identical): the towers run ONCE per clip and
the LLM keeps a KV cache, where the reference re-encodes the clip and re-runs the full sequence for every
generated token (generate(use_cache=False), R/model/VideoGLaMM.py:617-626,790-799;
R/model/videogpt_plus/model/language_model/llama3_1.py:110-134).
"""
import os

import torch

from . import ops

IMAGE_TOKEN_INDEX = -200  # R/model/videogpt_plus/constants.py


class VisionTowers:
    def __init__(self, params, cfg):
        self.P, self.cfg = params, cfg
        self.dtype = params.dtype

    # ------------------------------------------------------------------ shared
    def _patches(self, imgs, ps, wname, bias):
        """non-overlapping patch embedding as im2col + GEMM. imgs [B,3,H,W] NCHW -> [B, L, C]."""
        B, _, H, W = imgs.shape
        x = ops.permute5(imgs.contiguous(), (B, H, W, 3, 1), (3 * H * W, W, 1, H * W, 0)).view(B, H, W, 3)
        x = ops.cast(x, self.dtype)
        w = self.P.conv_w(wname)
        cols, Ho, Wo = ops.im2col(x, ps, ps, ps, 0, w.shape[1])
        return ops.linear(cols, w, bias).view(B, Ho * Wo, -1)

    # ------------------------------------------------------------------ L1 InternVideo2
    def iv2(self, video):
        """InternVideo2_Stage2V.forward / PretrainInternVideo2.forward(x_vis_return_idx=-2, x_vis_only=True)
        R/.../internvideo/utils.py:229-238; internvideo2.py:585-651,190-209,265-316.
        video [nc,4,3,H,W] -> [nc, 4*L, C] (CLS already dropped, arch.py:145)."""
        p, c = "model.vision_tower.vision_encoder.", self.cfg["iv2"]
        nc, T = video.shape[:2]
        heads = c["num_heads"]
        x = self._patches(video.reshape(nc * T, *video.shape[2:]), c["patch_size"], p + "patch_embed.proj", self.P.b(p + "patch_embed.proj"))
        C = x.shape[-1]
        x = x.view(nc, -1, C)
        cls = self.P.t(p + "cls_token").view(1, 1, C).expand(nc, 1, C)
        x = ops.add(torch.cat([cls, x], dim=1).contiguous(), self.P.t(p + "pos_embed").view(-1))
        n, hd = x.shape[1], C // heads
        for i in range(c["depth"] - 1):  # the loop breaks after block depth-2 (internvideo2.py:640-642)
            b = f"{p}blocks.{i}."
            h = ops.rmsnorm(x, self.P.f32(b + "norm1.weight"), 1e-6)
            qkv = ops.linear(h, self.P.w(b + "attn.qkv")).view(nc * n, 3 * C)
            q = ops.rmsnorm(qkv[:, :C], self.P.f32(b + "attn.q_norm.weight"), 1e-6).view(nc, n, heads, hd)
            k = ops.rmsnorm(qkv[:, C:2 * C], self.P.f32(b + "attn.k_norm.weight"), 1e-6).view(nc, n, heads, hd)
            v = qkv.view(nc, n, 3, heads, hd)[:, :, 2]
            o = ops.attention(q, k, v, hd ** -0.5).view(nc, n, C)
            x = ops.linear(o, self.P.w(b + "attn.proj"), self.P.b(b + "attn.proj"), gamma=self.P.f32(b + "ls1.gamma"), residual=x)
            h = ops.rmsnorm(x, self.P.f32(b + "norm2.weight"), 1e-6)
            h = ops.linear(h, self.P.w(b + "mlp.fc1"), self.P.b(b + "mlp.fc1"), act=ops.ACT_GELU)
            x = ops.linear(h, self.P.w(b + "mlp.fc2"), self.P.b(b + "mlp.fc2"), gamma=self.P.f32(b + "ls2.gamma"), residual=x)
        return x[:, 1:]

    # ------------------------------------------------------------------ L2 CLIP
    def clip(self, images):
        """CLIPVisionTower.forward('patch'): HF CLIPVisionModel hidden_states[-2] minus CLS —
        R/.../multimodal_encoder/clip_encoder.py:34-72.  images [T,3,H,W] -> [T, L, C]."""
        c = self.cfg["clip"]
        p = "model.image_vision_tower.vision_tower."
        v = p + "vision_model." if self.P.has(p + "vision_model.embeddings.class_embedding") else p
        heads = c["num_heads"]
        x = self._patches(images, c["patch_size"], v + "embeddings.patch_embedding", None)
        T, L, C = x.shape
        cls = self.P.t(v + "embeddings.class_embedding").view(1, 1, C).expand(T, 1, C)
        x = ops.add(torch.cat([cls, x], dim=1).contiguous(), self.P.t(v + "embeddings.position_embedding.weight").view(-1))
        x = ops.layernorm(x, self.P.f32(v + "pre_layrnorm.weight"), self.P.f32(v + "pre_layrnorm.bias"), 1e-5)
        n, hd = L + 1, C // heads
        for i in range(c["num_layers"] - 1):  # select_layer=-2: the last layer's output is never read
            b = f"{v}encoder.layers.{i}."
            h = ops.layernorm(x, self.P.f32(b + "layer_norm1.weight"), self.P.f32(b + "layer_norm1.bias"), 1e-5)
            wqkv, bqkv = self.P.fused([b + "self_attn.q_proj", b + "self_attn.k_proj", b + "self_attn.v_proj"])
            qkv = ops.linear(h, wqkv, bqkv).view(T, n, 3, heads, hd)
            o = ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], hd ** -0.5).view(T, n, C)
            x = ops.linear(o, self.P.w(b + "self_attn.out_proj"), self.P.b(b + "self_attn.out_proj"), residual=x)
            h = ops.layernorm(x, self.P.f32(b + "layer_norm2.weight"), self.P.f32(b + "layer_norm2.bias"), 1e-5)
            h = ops.linear(h, self.P.w(b + "mlp.fc1"), self.P.b(b + "mlp.fc1"), act=ops.ACT_QUICK_GELU)
            x = ops.linear(h, self.P.w(b + "mlp.fc2"), self.P.b(b + "mlp.fc2"), residual=x)
        return x[:, 1:]

    # ------------------------------------------------------------------ L3 adapters + pooling
    def _projector(self, name, x):
        """'linear' or 'mlpNx_gelu' — R/.../multimodal_projector/builder.py:17-54."""
        if self.P.has(name + ".weight"):
            return ops.linear(x, self.P.w(name), self.P.b(name))
        i = 0
        while self.P.has(f"{name}.{i + 2}.weight"):
            x = ops.linear(x, self.P.w(f"{name}.{i}"), self.P.b(f"{name}.{i}"), act=ops.ACT_GELU)
            i += 2
        return ops.linear(x, self.P.w(f"{name}.{i}"), self.P.b(f"{name}.{i}"))

    def encode(self, images, context_images, comm=None):
        """encode_videos + project(input_type='video') — R/model/videogpt_plus/model/arch.py:121-151,164-191.
        images [Te,3,224,224], context [Te,3,336,336] -> visual tokens [Te*144 + Te*64, D] (context first);
        context_images None: images [t,3,336,336] -> [t*576, D].
        comm (dist.FrameSharder, world > 1): this rank encodes only its block of CLIP frames and of 4-frame InternVideo2
        chunks; the projected, pooled tokens are all-gathered (every op up to there is per frame / per chunk)."""
        if context_images is None:
            # image prompt (encode_images + project(input_type="image"), arch.py:110-119,393-397): CLIP patch features of
            # the image(s) -> image_mm_projector, no pooling, all tokens concatenated
            cf = self._projector("model.image_mm_projector", self.clip(images).contiguous())
            return cf.view(-1, cf.shape[-1])
        te = images.shape[0]
        assert te % 4 == 0, "the video encoder consumes 4-frame chunks (arch.py:133)"
        video = images.view(te // 4, 4, *images.shape[1:])
        # opt-in (VG_TOWERS_SHARDED=1): a rank that encodes fewer frames runs GEMMs of another M, which can take another tile route
        # (another fp32 summation order): in bf16 the visual tokens — and with them greedy ids — may then differ from the
        # single-GPU run.  The default keeps the whole LLM side replicated: N-GPU ids == 1-GPU ids by construction.
        sharded = comm is not None and comm.world > 1 and os.environ.get("VG_TOWERS_SHARDED", "0") == "1"
        if sharded:
            c0, cn = comm.block(te)
            v0, vn = comm.block(te // 4)
            context_images, video = context_images[c0:c0 + cn], video[v0:v0 + vn]
        else:
            cn, vn = te, te // 4

        def video_tokens():
            if vn == 0:
                return None
            vf = self._projector("model.mm_projector", self.iv2(video).contiguous())      # [nc, 4*L, D]
            D = vf.shape[-1]
            g = int(round((vf.shape[1] // 4) ** 0.5))
            # arch.py:173,177-178 hard-code 8x8 / 12x12 outputs; with the 16x16 / 24x24 token grids of the shipped
            # towers adaptive_avg_pool2d is exactly a 2x2 mean
            assert g == 16, "the video token grid must be 16x16"
            return ops.pool2(vf.view(vn * 4, g, g, D), False).view(-1, D)                 # 16x16 -> 8x8 per frame

        def context_tokens():
            if cn == 0:
                return None
            cf = self._projector("model.image_mm_projector", self.clip(context_images).contiguous())   # [Te, Lc, D]
            D = cf.shape[-1]
            g = int(round(cf.shape[1] ** 0.5))
            assert g == 24, "the context token grid must be 24x24"
            return ops.pool2(cf.view(cn, g, g, D), False).view(-1, D)                      # 24x24 -> 12x12 per frame

        if images.is_cuda and os.environ.get("VG_TOWERS_OVERLAP", "1") != "0" and vn and cn:
            # the two towers are independent and their GEMMs are small (M = 2050 / 4616 rows: ~1 round of tiles with a
            # long tail each): InternVideo2 goes to a second stream so that the tails of one fill under the other
            if getattr(self, "_side", None) is None:
                self._side = torch.cuda.Stream(device=images.device)
            main = torch.cuda.current_stream(images.device)
            self._side.wait_stream(main)
            with torch.cuda.stream(self._side):
                vf = video_tokens()
            cf = context_tokens()
            main.wait_stream(self._side)
            vf.record_stream(main)
        else:
            vf = video_tokens()
            cf = context_tokens()
        if sharded:
            D = self.P.sd["model.embed_tokens.weight"].shape[1]          # the projectors end in the LLM width
            cf = comm.gather_rows(cf, te, 144, (D,), self.P.dtype, images.device)
            vf = comm.gather_rows(vf, te // 4, 4 * 64, (D,), self.P.dtype, images.device)
        return torch.cat([cf, vf], dim=0)


def decode_gemv_mode(value, decode_weights, dtype, env, step, projections, supported, quant_projections=(), quant_supported=None):
    """cfg["llm"]["decode_gemv"]: False for None / "valu" (the decode GEMVs of DESIGN 5d / 11), True for "mfma" (every plain projection of the
    single-row and the B-row step on vg_decode_gemm_rows), "mfma_q" for "mfma_q" (the same step with fp8 / mxfp4 decode weights: the
    quantised projections on vg_decode_gemm_w8_rows / vg_decode_gemm_w4_rows, the bf16 ones on vg_decode_gemm_rows) — or a ValueError that names
    why this decoder cannot take the mode.
    decode_weights: cfg["llm"]["decode_weights"]; dtype: the model's; env: the environment; step: "rope" (Llama-3 width: q|k|v + RoPE + append
    stays on its own kernel), "attention" (Phi-3-mini width: the q|k|v GEMV moves too) or None (neither B-row step covers the decoder);
    projections: the (N, K) of the bf16 weights the mode moves; supported: ops.decode_gemm_rows_supported.  "mfma_q" only: quant_projections: the
    (N, K, kind, norm) of the quantised weights — kind "w8" | "w4", norm: the projection runs behind a fused RMSNorm — and quant_supported:
    {"w8": ops.decode_gemm_w8_rows_supported, "w4": ops.decode_gemm_w4_rows_supported}.  Pure: no device work."""
    if value in (None, "valu"):
        return False
    if value not in ("mfma", "mfma_q"):
        raise ValueError(f"cfg['llm']['decode_gemv'] = {value!r}: 'valu' (default), 'mfma' or 'mfma_q'")
    if value == "mfma" and decode_weights in ("fp8", "mxfp4"):
        raise ValueError(f"decode_gemv = 'mfma' streams the bf16 weights: it does not combine with decode_weights = {decode_weights!r} "
                         "(decode_gemv = 'mfma_q' does)")
    if value == "mfma_q" and decode_weights not in ("fp8", "mxfp4"):
        raise ValueError(f"decode_gemv = 'mfma_q' streams fp8 / mxfp4 decode weights, not decode_weights = {decode_weights!r}: with bf16 weights "
                         "the mode is decode_gemv = 'mfma'")
    if dtype != torch.bfloat16:
        raise ValueError(f"decode_gemv = {value!r} needs a bf16 model (v_mfma_f32_16x16x32_bf16), not {dtype}")
    for knob in ("VG_DECODE_CHAIN", "VG_DECODE_AHEAD"):
        if env.get(knob, "0") != "0":
            raise ValueError(f"decode_gemv = {value!r} does not combine with {knob}={env.get(knob)}")
    if step not in ("rope", "attention"):
        raise ValueError(f"decode_gemv = {value!r}: this decoder takes neither the rope step (Llama-3 width) nor the decode_attention rows step (Phi-3-mini width)")
    for N, K in projections:
        if not supported(N, K):
            raise ValueError(f"decode_gemv = {value!r}: vg_decode_gemm_rows does not cover a [{N}, {K}] projection (uncovered width)")
    if value == "mfma":
        return True
    for N, K, kind, norm in quant_projections:
        if not quant_supported[kind](N, K):
            raise ValueError(f"decode_gemv = 'mfma_q': vg_decode_gemm_{kind}_rows does not cover a [{N}, {K}] projection (uncovered width)")
        if norm and K > 4096:
            raise ValueError(f"decode_gemv = 'mfma_q': the RMSNorm-fused form of vg_decode_gemm_{kind}_rows exists at K <= 4096 only, "
                             f"not for the [{N}, {K}] projection behind the norm (hidden {K})")
    return "mfma_q"


def prefill_gemm_mode(value, decode_weights, dense_mlp, dtype, hidden, ffn):
    """cfg["llm"]["prefill_gemm"] and cfg["llm"]["dense_mlp"] -> (mode, drop).  mode: "mxfp4" (the MLP of the prefill on the packed MXFP4 rows the
    decode step streams: vg_gemm_w4a8 on the tile path, vg_decode_gemv_w4_rows for short prefills; q|k|v and o on vg_gemm_f8), "fp8"
    (every GEMM of the tile path on vg_gemm_f8) or None — any other value keeps the dense GEMMs of the model dtype.  drop: dense_mlp = "drop",
    the decoder builds the packed rows of every layer and lets go of the dense gate / up / down weights (Params.drop); valid only when neither the
    prefill nor the decode step would read them, a ValueError names the reader otherwise.  decode_weights: cfg["llm"]["decode_weights"]; dtype: the
    model's; hidden, ffn: the MLP's widths.  Pure: no device work."""
    if dense_mlp not in (None, "keep", "drop"):
        raise ValueError(f"cfg['llm']['dense_mlp'] = {dense_mlp!r}: 'keep' (default) or 'drop'")
    drop = dense_mlp == "drop"
    if value != "mxfp4":
        if drop:
            raise ValueError(f"dense_mlp = 'drop': the prefill (prefill_gemm = {value!r}) still reads the dense MLP weights; "
                             "it needs prefill_gemm = 'mxfp4' and decode_weights = 'mxfp4'")
        return ("fp8" if value == "fp8" else None), False
    if dtype != torch.bfloat16:
        raise ValueError(f"prefill_gemm = 'mxfp4' needs a bf16 model (e4m3 activations x MXFP4 weights with bf16 rows between the GEMMs), not {dtype}")
    if hidden not in (3072, 4096, 8192) or ffn not in (8192, 14336):
        raise ValueError(f"prefill_gemm = 'mxfp4': no packed MXFP4 row of length hidden = {hidden} / ffn = {ffn} "
                         "(hidden 3072, 4096 or 8192 and ffn 8192 or 14336)")
    if drop and decode_weights != "mxfp4":
        raise ValueError(f"dense_mlp = 'drop': the decode step (decode_weights = {decode_weights!r}) still reads the dense MLP weights; "
                         "it needs prefill_gemm = 'mxfp4' and decode_weights = 'mxfp4'")
    return "mxfp4", drop


def kv_cache_mode(value, dtype, device_type, fused, env):
    """cfg["llm"]["kv_cache"] -> truthy when the decode step keeps its keys / values as e4m3 codes: True for "fp8" (the
    decode_attention form of the step at every width), the string "rope" for "fp8_rope" (the same format on the rope step: Llama-3 width);
    False for "bf16" (the default: the cache holds the model's dtype), or ValueError saying why this decoder cannot take the mode.  dtype /
    device_type: the model's; fused: the fused decode kernels cover the decoder (LlamaDecoder.fused_decode); env: the environment.  Pure: no
    device work."""
    if value in (None, "bf16"):
        return False
    if value not in ("fp8", "fp8_rope"):
        raise ValueError(f"cfg['llm']['kv_cache'] = {value!r}: 'bf16' (default), 'fp8' or 'fp8_rope'")
    if dtype != torch.bfloat16:
        raise ValueError(f"kv_cache = {value!r} needs a bf16 model (the e4m3 cache holds quantised bf16 rows), not {dtype}")
    if device_type != "cuda":
        raise ValueError(f"kv_cache = {value!r} runs on the GPU's decode kernels, not on device {device_type!r}")
    if not fused:
        raise ValueError(f"kv_cache = {value!r} needs the fused decode kernels (vg_decode_attention_kv8 / vg_decode_attention2_kv8): this decoder's "
                         "shape is outside them, or VG_DECODE_FUSED=0")
    if env.get("VG_DECODE_CHAIN", "0") != "0":
        raise ValueError(f"kv_cache = {value!r} does not combine with VG_DECODE_CHAIN={env.get('VG_DECODE_CHAIN')}: vg_decode_layer reads a bf16 cache")
    return True if value == "fp8" else "rope"


def decode_step_form(rope_covered, attn_rows_covered, kv8=False):
    """"rope" | "attention" | None: which B-row step (RowsDecode) goes with the decoder's single-row step.  rope_covered: the single-row step may
    take the rope path (bf16 head_dim 128: Llama-3 width); attn_rows_covered: the B-row kernels cover the decode_attention step's layer (Phi-3-mini
    width).  kv8 = kv_cache_mode's answer.  True (kv_cache = "fp8"): that mode keeps off the rope path, so Llama-3 width runs the decode_attention
    form single-row and has no B-row step — the mode is meant for the MHA model.  "rope" (kv_cache = "fp8_rope"): the mode IS the rope step on
    e4m3 caches (rope_covered then speaks of ops.decode_rope_path_kv8) and has no other form: None where that step does not cover the decoder
    (kv_cache_check_rope refuses such a decoder).  Pure."""
    if kv8 == "rope":
        return "rope" if rope_covered else None
    if rope_covered and not kv8:
        return "rope"
    return "attention" if attn_rows_covered else None


def kv_cache_check_rope(step):
    """ValueError when kv_cache = "fp8_rope" meets a decoder its step does not cover.  step: decode_step_form(..., kv8="rope").  Pure."""
    if step != "rope":
        raise ValueError("kv_cache = 'fp8_rope' is the fp8 K/V cache on the rope step (vg_decode_qkv_rope_kv8 + vg_decode_attention2_kv8: bf16, "
                         "head_dim 128, hidden 2048 / 4096 — Llama-3 width), which does not cover this decoder (Phi-3-mini width, or "
                         "VG_DECODE_ROPE=0): kv_cache = 'fp8' runs the decode_attention form of the step at every width")


def kv_cache_check_gemv(decode_gemv, step):
    """ValueError when cfg["decode_gemv"] needs a step the fp8-K/V decoder no longer has: the MFMA modes run the B-row kernels in the single-row step
    too, and at Llama-3 width those belong to the rope step.  step: decode_step_form(..., kv8=True).  Pure."""
    if decode_gemv in ("mfma", "mfma_q") and step is None:
        raise ValueError(f"kv_cache = 'fp8' does not combine with decode_gemv = {decode_gemv!r} on this decoder: the mode's projections belong to "
                         "the rope step (Llama-3 width), which this mode keeps off (kv_cache = 'fp8_rope' is that step on e4m3 caches); Phi-3-mini "
                         "width (the decode_attention rows step) takes both")


class DecodeProjections:
    """Which ops entry point, which stored form of the weight and which [N, K] each projection of the LLM decode step takes — the one place where
    the modes meet.  Roles: "qkv" (the decode_attention step only: the rope step keeps q|k|v inside decode_qkv_rope), "o",
    "gate_up", "down", "lm_head".

    Stored form (fmt): q|k|v and o are bf16 in every mode; gate|up and down follow cfg["decode_weights"] ("bf16" | "w8" = fp8 e4m3 + row scales |
    "w4" = packed MXFP4 rows); the lm_head is fp8 under either quantised format (it decides the token ids and is 4 % of the bytes), else bf16.
    Entry point: KERNELS[fmt], picked by cfg["decode_gemv"] and by whether the step is the single-row one (LlamaDecoder) or the B-row one
    (RowsDecode, rows=True): under "mfma" / "mfma_q" both steps run the MFMA B-row kernels (B = 1 in the single-row step).  The bf16 lm_head of
    the VALU modes is a plain ops.linear.  Entries are held as names and looked up in ops at call time.
    self.pack: the bf16 MLP roles whose VALU single-row step hands ops.decode_gemv the lossless 13-bit rows of the same weights to stream
    (p13=; VG_DECODE_PACK): entry point, stored form and bits stay decode_gemv's on the bf16 weight, so the B-row step, weights()
    and covered() see no difference.
    gate_up runs behind the fused post_attention_layernorm with SwiGLU, qkv behind input_layernorm; o and down add the residual; the lm_head
    gives fp32 logits."""
    #          fmt      VALU single-row    VALU B-row             MFMA, either step
    KERNELS = {"bf16": ("decode_gemv",    "decode_gemv_rows",    "decode_gemm_rows"),
               "w8":   ("decode_gemv_w8", "decode_gemv_w8_rows", "decode_gemm_w8_rows"),
               "w4":   ("decode_gemv_w4", "decode_gemv_w4_rows", "decode_gemm_w4_rows")}
    # (role, K) whose VALU single-row decode_gemv streams the 13-bit rows of its bf16 weight.  VG_DECODE_PACK unset: these, the shapes
    # where that measured faster than streaming the bf16 weight; "1": wherever the kernel exists; "0": nowhere
    PACK_DEFAULT = {("gate_up", 4096), ("down", 14336)}
    PACK_K = (4096, 14336)       # vg_decode_gemv_p13_supported, held here so that the table stays pure

    def __init__(self, decode_gemv, decode_weights, hidden=0, ffn=0, vocab=0, qkv=0, attn=None, step=None, env=None, pack=True):
        """decode_gemv / decode_weights: the cfg values; hidden, ffn, vocab, qkv (rows of q|k|v), attn (heads x head_dim: o's K; default hidden):
        the widths weights() reports; step: "rope" | "attention" | None as decode_gemv_mode's; env: the environment (VG_DECODE_PACK; default
        os.environ); pack=False: no 13-bit rows (a model that is not bf16).  Pure: no device work."""
        self.mfma = decode_gemv in ("mfma", "mfma_q")
        mlp = {"fp8": "w8", "mxfp4": "w4"}.get(decode_weights, "bf16")
        self.fmt = dict(qkv="bf16", o="bf16", gate_up=mlp, down=mlp, lm_head="bf16" if mlp == "bf16" else "w8")
        attn = hidden if attn is None else attn
        # role -> (N, K, behind a fused RMSNorm), in the order decode_gemv_mode is asked (gate|up: N per half)
        self.shape = dict(o=(hidden, attn, False), gate_up=(ffn, hidden, True), down=(hidden, ffn, False), lm_head=(vocab, hidden, False))
        if step == "attention":
            self.shape["qkv"] = (qkv, hidden, True)
        # the MLP roles whose single-row step runs on the 13-bit rows: VALU mode, bf16 decode weights, Llama widths (both row lengths covered)
        knob = (os.environ if env is None else env).get("VG_DECODE_PACK", "")
        self.pack = {r for r in ("gate_up", "down")
                     if pack and mlp == "bf16" and not self.mfma and knob != "0" and {hidden, ffn} == set(self.PACK_K)
                     and (knob == "1" or (r, self.shape[r][1]) in self.PACK_DEFAULT)}

    def entry(self, role, rows=False):
        """the name of the ops function that runs `role` in the single-row (rows=False) or the B-row step"""
        if role == "lm_head" and self.fmt[role] == "bf16" and not self.mfma:
            return "linear"
        return self.KERNELS[self.fmt[role]][2 if self.mfma else int(bool(rows))]

    def weights(self, quantised=None):
        """[(N, K, fmt, norm)] of the step's weights; quantised=False: the bf16 ones only, True: the fp8 / MXFP4 ones only"""
        return [(N, K, self.fmt[r], norm) for r, (N, K, norm) in self.shape.items()
                if quantised is None or quantised == (self.fmt[r] != "bf16")]

    def covered(self, N, K, fmt, rows=True):
        """True when the entry point of a [N, K] weight stored as fmt has that shape (the VALU GEMVs are asked by row length alone)"""
        sup = getattr(ops, self.KERNELS[fmt][2 if self.mfma else int(bool(rows))] + "_supported")
        return sup(N, K) if self.mfma else sup(K)

    def operands(self, P, role, l="", packed=False):
        """the weight operands of `role` in layer prefix l ("model.layers.3."), in the role's stored form: one tensor, or fp8's (codes, scales);
        packed (a role of self.pack in the single-row step): the bf16 tensor, then its 13-bit rows, scales and raw rows — or the bf16 tensor alone
        where the matrix is over the raw-row cap"""
        names, stored = {"qkv": ([l + "self_attn.q_proj", l + "self_attn.k_proj", l + "self_attn.v_proj"], l + "self_attn.qkv_proj"),
                         "o": (l + "self_attn.o_proj", None), "gate_up": ([l + "mlp.gate_proj", l + "mlp.up_proj"], l + "mlp.gate_up_proj"),
                         "down": (l + "mlp.down_proj", None), "lm_head": ("lm_head", None)}[role]
        fmt = self.fmt[role]
        if fmt == "w8":
            return P.fp8(names, stored=stored)
        if fmt == "w4":
            return (P.fp4(names, stored=stored),)
        w = P.w(names) if stored is None else P.fused(names, stored=stored)[0]
        return (w,) + ((P.p13(names, stored=stored) or ()) if packed else ())

    def run(self, role, rows, P, l, x, **kw):
        """launch `role` on x: kw = the entry point's norm_w / eps / glu / residual / out_dtype"""
        if role in self.pack and not rows:
            w, *p13 = self.operands(P, role, l, packed=True)
            return getattr(ops, self.entry(role, rows))(x, w, p13=tuple(p13) or None, **kw)
        return getattr(ops, self.entry(role, rows))(x, *self.operands(P, role, l), **kw)

    def mlp(self, rows, P, l, x, eps):
        """norm + gate|up + SwiGLU, then down + residual: the two MLP launches of a layer -> (the SwiGLU rows, the layer's output).  The caller
        holds the SwiGLU rows until the next layer's: released here, the captured step lays its buffers out otherwise (measured: the B = 8 mfma_q
        step 4.42 instead of 4.41 ms)"""
        a = self.run("gate_up", rows, P, l, x, norm_w=P.f32(l + "post_attention_layernorm.weight"), eps=eps, glu=True)
        return a, self.run("down", rows, P, l, a, residual=x)

    def lm_head(self, rows, P, h):
        """fp32 logits of the final-norm rows h (the single-row kernels take a contiguous row)"""
        name = self.entry("lm_head", rows)
        return getattr(ops, name)(h if rows or name == "linear" else h.contiguous(), *self.operands(P, "lm_head"), out_dtype=torch.float32)


class LlamaDecoder:
    """HF LlamaModel / Phi3Model arithmetic (RMSNorm, rotate-half RoPE, GQA attention, SwiGLU) with a KV cache.  Phi-3 (the
    released checkpoint's LLM, R/model/videogpt_plus/model/language_model/phi3.py:29-40) is the same graph with the
    q|k|v and gate|up projections already fused in the checkpoint, and a sliding window: with cfg["sliding_window"] = w (2047 for
    Phi-3-mini-4k) position i attends to positions [i - w, i] — w + 1 keys, the mask transformers==4.41.0 (the reference's pin) builds
    in modeling_attn_mask_utils._make_causal_mask (diagonal = -w - 1) and its flash-attention path (window_size = (w, w)) — applied
    inside the prefill and decode attention kernels.  The released model at the reference's default NUM_FRAMES = 16 (S ~ 3370) needs it.

    Prefill runs eagerly (sequence length varies per clip).  A decode step is fully static — the token id, the
    cache position and the KV length all live in device memory (tok_dev / pos_dev) — so it is captured ONCE into
    a HIP graph (torch.cuda.CUDAGraph around the same C-ABI launches) and replayed per generated token: ~330
    kernel launches per token stop costing host time.  One instance is kept per model and max_len bucket."""
    HIST = 4096      # generated tokens per clip the device-side history holds (the reference's chat caps max_new_tokens at 512)

    def __init__(self, params, cfg, max_len, use_graph=None):
        self.P, self.c = params, cfg
        c = cfg
        self.D, self.H, self.Hkv = c["hidden"], c["num_heads"], c["num_kv_heads"]
        self.hd = self.D // self.H
        self.max_len = max_len
        self.window = int(c["sliding_window"]) + 1 if c.get("sliding_window") else 0     # visible keys, own position included
        dev, dt = params.device, params.dtype
        # zero-filled: vg_decode_attention2 masks rows past the position instead of skipping them (every row must hold finite values)
        self.kc = [torch.zeros(max_len, self.Hkv, self.hd, dtype=dt, device=dev) for _ in range(c["num_layers"])]
        self.vc = [torch.zeros(max_len, self.Hkv, self.hd, dtype=dt, device=dev) for _ in range(c["num_layers"])]
        inv = 1.0 / (c["rope_theta"] ** (torch.arange(0, self.hd, 2, dtype=torch.int64).float() / self.hd))
        fr = torch.arange(max_len).float()[:, None] * inv[None]
        self.cos = fr.cos().to(dev).contiguous()
        self.sin = fr.sin().to(dev).contiguous()
        self.pos = 0
        self.pos_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.tok_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        # device-side loop state (vg_decode_advance): step counter, emitted / raw (pre-forcing) token history, forced-token table
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.hist = torch.zeros(self.HIST, dtype=torch.int64, device=dev)
        self.raw = torch.zeros(self.HIST, dtype=torch.int64, device=dev)
        self.forced = torch.full((self.HIST,), -1, dtype=torch.int64, device=dev)
        self.rope_cs = torch.zeros(self.hd, dtype=torch.float32, device=dev)     # [cos row | sin row] of *pos_dev for vg_decode_qkv_rope
        self.amax_acc = torch.zeros(1, dtype=torch.int64, device=dev)            # vg_argmax_partial's accumulator (vg_decode_step_end leaves it zero)
        self.hid_all = torch.empty(max_len, self.D, dtype=dt, device=dev)   # final-norm state of every position
        self.use_graph = (dev.type == "cuda") if use_graph is None else use_graph
        self.graph, self.graphs = None, {}
        self.kpw, self.kpw_min = 0, int(os.environ.get("VG_DEC_KPW_MIN", "2048"))
        self.attn_ws = None
        es = 2 if dt == torch.bfloat16 else 4
        # (params.ffn: the width an earlier decoder on these Params noted when it dropped the dense MLP weights, dense_mlp = "drop")
        ffn = c.get("ffn") or params.ffn or params.t("model.layers.0.mlp.down_proj.weight").shape[1]
        self.ffn = ffn
        # the fused decode kernels' shape limits (vg_decode_gemv / vg_decode_attention); VG_DECODE_FUSED=0 = A/B knob
        # fp8 (e4m3) weights with per-row scales in the decode step's MLP GEMVs and the lm_head (cfg["decode_weights"] == "fp8": the decode
        # side of BASELINE config C4's "fp8 LLM path"; bf16 activations, fp32 accumulation; the prefill GEMMs stay bf16)
        self.w8 = c.get("decode_weights") == "fp8"
        # MXFP4 weights (e2m1 codes, one e8m0 scale per 32 K elements) in the decode step's MLP GEMVs (cfg["decode_weights"] == "mxfp4"); the lm_head
        # takes the fp8 GEMV (it decides the token ids and is 4 % of the remaining bytes), the attention projections stay bf16 as under "fp8"
        self.w4 = c.get("decode_weights") == "mxfp4"
        # fp8 MFMA prefill GEMMs (cfg["prefill_gemm"] == "fp8"): vg_quantize_fp8_rows + vg_gemm_f8; the attention itself stays bf16
        # cfg["prefill_gemm"] == "mxfp4": the MLP of the prefill on the packed MXFP4 rows (vg_gemm_w4a8; q|k|v and o as under "fp8"), and
        # cfg["dense_mlp"] == "drop": no dense gate / up / down weights are kept (prefill_gemm_mode; the packed rows are built at the end of __init__)
        pmode, self.dense_dropped = prefill_gemm_mode(c.get("prefill_gemm"), c.get("decode_weights"), c.get("dense_mlp"), dt, self.D, ffn)
        self.w4_prefill = pmode == "mxfp4"
        self.check_dense(c)
        self.f8_prefill = pmode == "fp8"
        assert not self.f8_prefill or dt == torch.bfloat16, "the fp8 prefill pairs with a bf16 model"
        if self.w8:
            assert dt == torch.bfloat16 and self.D in (3072, 4096, 8192) and ffn in (8192, 14336), "fp8 decode weights: bf16 model, supported row lengths"
        self.fused_decode = (os.environ.get("VG_DECODE_FUSED", "1") != "0" and (self.H // self.Hkv) in (1, 2, 4, 8)
                             and self.hd % (16 // es) == 0 and self.hd * es <= 512 and max_len <= 8192
                             and max(self.D, ffn) * es <= 65536 and self.D % (16 // es) == 0 and ffn % (16 // es) == 0)
        if self.w4:
            assert dt == torch.bfloat16 and self.D in (3072, 4096, 8192) and ffn in (8192, 14336), "mxfp4 decode weights: bf16 model, supported row lengths"
        assert self.fused_decode or not (self.w8 or self.w4), "fp8 / mxfp4 decode weights need the fused decode kernels"
        # vg_decode_layer: which roles of a layer run as one chained launch.  VG_DECODE_CHAIN=1 (attention + o_proj) / 3 (+ the MLP); default 0 =
        # separate launches: measured on C2 the chained launch only ties (27.4 us vs 20.1 + 8.0; 85.4 vs 84.7 for the whole layer — every
        # device-side hand-off is a fabric round trip, as the launch boundary it replaces is)
        self.chain_roles, self.chain_flags, self.chain_err = 0, None, None
        # cfg["kv_cache"] == "fp8" (DESIGN 8c): the decode step reads and appends e4m3 keys / values (kc8 / vc8: one byte per element, no scale, the
        # bf16 cache's layout); kc / vc stay as the prefill's bf16 staging — a prefill attends to unquantised K/V with today's launches, then
        # forward() quantises the rows it wrote.  No chained launch.  "fp8": the step is the decode_attention form at every width (kv8 is True: the
        # new token's K/V take part in their own step unquantised).  "fp8_rope": the rope step on the same caches (kv8 == "rope": the new token's
        # row is in the cache before the attention reads it, so it attends to its own K/V quantised); a decoder that step does not cover is refused
        self.kv8 = kv_cache_mode(c.get("kv_cache"), dt, dev.type, self.fused_decode, os.environ)
        self.kc8 = self.vc8 = None
        self.staged = 0      # kv8: rows [0, staged) of kc / vc are what a prefill wrote; decode steps append to kc8 / vc8 only (forward())
        if self.fused_decode and dev.type == "cuda" and not self.kv8:
            self.chain_roles = min(ops.decode_layer_roles(self.H, self.Hkv, self.hd, self.D, ffn, dt), int(os.environ.get("VG_DECODE_CHAIN", "0")))
            if self.chain_roles == 2:
                self.chain_roles = 1
        # r06: RoPE + KV append in the q|k|v GEMV's epilogue, attention as a wave-private flash pass (bf16, head_dim 128); VG_DECODE_ROPE=0 = A/B knob
        rope_shapes = ops.decode_rope_path_kv8 if self.kv8 == "rope" else ops.decode_rope_path
        rope_covered = (self.fused_decode and dev.type == "cuda" and not self.chain_roles and os.environ.get("VG_DECODE_ROPE", "1") != "0"
                        and rope_shapes(self.H, self.Hkv, self.hd, self.D, dt))
        rows_covered = (self.fused_decode and dev.type == "cuda" and not self.chain_roles
                        and ops.decode_step_rows_supported(self.H, self.Hkv, self.hd, self.D, ffn, dt))
        step = decode_step_form(rope_covered, rows_covered, self.kv8)
        if self.kv8 == "rope":
            kv_cache_check_rope(step)
        if self.kv8:
            self.kc8 = [torch.zeros(max_len, self.Hkv, self.hd, dtype=torch.uint8, device=dev) for _ in range(c["num_layers"])]
            self.vc8 = [torch.zeros(max_len, self.Hkv, self.hd, dtype=torch.uint8, device=dev) for _ in range(c["num_layers"])]
        self.rope_path = step == "rope"
        self.kpw2 = int(os.environ.get("VG_DEC2_KPW", "256"))
        # cfg["decode_gemv"] ("valu" | "mfma" | "mfma_q") x cfg["decode_weights"]: which kernel and stored weight each projection of the single-row
        # and the B-row step takes is DecodeProjections' answer; decode_gemv_mode refuses what this decoder cannot run before any launch
        if self.kv8:
            kv_cache_check_gemv(c.get("decode_gemv"), step)
        head = params.sd.get("lm_head.weight")       # (a decoder that only prefills may come without one)
        self.proj = DecodeProjections(c.get("decode_gemv"), c.get("decode_weights"), hidden=self.D, ffn=ffn, vocab=0 if head is None else head.shape[0],
                                      qkv=(self.H + 2 * self.Hkv) * self.hd, attn=self.H * self.hd, step=step, pack=dt == torch.bfloat16)
        mode = decode_gemv_mode(c.get("decode_gemv"), c.get("decode_weights"), dt, os.environ, step,
                                [(N, K) for N, K, _, _ in self.proj.weights(quantised=False)], ops.decode_gemm_rows_supported,
                                quant_projections=self.proj.weights(quantised=True),
                                quant_supported={"w8": ops.decode_gemm_w8_rows_supported, "w4": ops.decode_gemm_w4_rows_supported})
        # mfma: decode_gemv = "mfma" (bf16 weights); mfma_q: decode_gemv = "mfma_q" (fp8 / mxfp4 weights)
        self.mfma, self.mfma_q = mode is True, mode == "mfma_q"
        # sampled decoding (vg_sample): None = greedy; else dict(T, k, p, seed), the values held in the device block samp_params that
        # the captured step reads — a new temperature / top-p / top-k / seed is a copy into it, never a re-capture
        self.sampling, self.samp_params, self.samp_ws, self.samp_fast = None, None, None, False
        # per-token scores (vg_token_scores_rows): off by default; set_scores(True) makes every emitted token leave
        # (logprob, margin) in score_hist and (top1, top2) in top2_hist, at the slot of its step
        self.scores_on, self.score_hist, self.top2_hist, self.score_ws = False, None, None, None
        if self.dense_dropped:
            self._drop_dense_mlp()

    def check_dense(self, c):
        """RuntimeError when the dense MLP weights of these Params are gone (dense_mlp = "drop") and cfg c asks for a mode that reads them"""
        if self.P.dropped and (c.get("prefill_gemm") != "mxfp4" or c.get("decode_weights") != "mxfp4"):
            reader = f"the prefill (prefill_gemm = {c.get('prefill_gemm')!r})" if c.get("prefill_gemm") != "mxfp4" else \
                f"the decode step (decode_weights = {c.get('decode_weights')!r})"
            raise RuntimeError(f"the dense MLP weights of this model were dropped (dense_mlp = 'drop'): {reader} would read them; "
                               "keep prefill_gemm = decode_weights = 'mxfp4' or load the checkpoint again")

    def _drop_dense_mlp(self):
        """dense_mlp = "drop": layer by layer, the packed MXFP4 rows, then the layer's dense gate / up / down tensors leave the state dict and the
        cache — at no moment does more than one layer hold its concatenated gate|up copy and the quantiser's temporaries beside the packed rows"""
        P = self.P
        P.ffn = self.ffn
        for i in range(self.c["num_layers"]):
            l = f"model.layers.{i}."
            gu = [l + "mlp.gate_proj", l + "mlp.up_proj"]
            P.fp4(gu, stored=l + "mlp.gate_up_proj")
            P.fp4(l + "mlp.down_proj")
            P.drop(gu + [l + "mlp.gate_up_proj", l + "mlp.down_proj"])

    def reset(self):
        self.pos = 0
        self.pos_dev.zero_()
        self.step_dev.zero_()
        # a step that stopped between the token hand-off and its decode (an exception in a hook, an aborted clip) must not leave its key or its
        # forcing table to the next clip
        self.amax_acc.zero_()
        self.forced.fill_(-1)

    def set_sampling(self, sampling):
        """sampling = None (greedy) or dict(T=, k=, p=, seed=): HF's Temperature / TopK / TopP warpers and a Philox draw per step (ops.sample_partial)"""
        if sampling is None:
            self.sampling = None
            return
        if self.samp_params is None:
            self.samp_params = torch.zeros(6, dtype=torch.int32, device=self.P.device)
            self.samp_ws = ops.sample_workspace(self.P.device)
        self.sampling = dict(T=float(sampling["T"]), k=int(sampling["k"]), p=float(sampling["p"]), seed=int(sampling["seed"]))
        ops.sampling_params(self.sampling["T"], self.sampling["k"], self.sampling["p"], self.sampling["seed"], self.P.device, out=self.samp_params)
        # the route is fixed by k: the multi-workgroup fast route for 1 <= k <= 64, the one-workgroup general route otherwise
        self.samp_fast = ops.sample_fast_route(self.sampling["k"], self.P.t("lm_head.weight").shape[0])

    def set_scores(self, on):
        """on: every emitted token also records its log-probability, top-2 margin and top-2 indices (ops.token_scores_rows) at slot *step_dev
        of score_hist (float32 [HIST, 2]) / top2_hist (int64 [HIST, 2]); the step with scores is a captured graph of its own.  Off: the
        launches, graph keys and buffers of a decoder that never heard of scores."""
        self.scores_on = bool(on)
        if self.scores_on and self.score_hist is None:
            dev = self.P.device
            self.score_hist = torch.zeros(self.HIST, 2, dtype=torch.float32, device=dev)
            self.top2_hist = torch.zeros(self.HIST, 2, dtype=torch.int64, device=dev)
            self.score_ws = ops.token_scores_workspace(1, dev)

    def _record_scores(self, logits, acc=None, tok=None):
        """the scores launch on the fp32 logits row [1, V] of the token being emitted (slot *step_dev)"""
        ops.token_scores_rows(logits, self.step_dev, self.score_hist.view(1, self.HIST, 2), self.top2_hist.view(1, self.HIST, 2), acc=acc, tok=tok,
                              ws=self.score_ws)

    def _layers(self, x, pos0, pos_dev, kv_hook=None):
        """decoder stack on x [S,D]; KV appended at pos (host value pos0, or *pos_dev when given).
        kv_hook(i): called after layer i wrote its K/V rows and before its attention (the sequence-parallel prefill
        all-gathers the other ranks' rows there)."""
        P, c = self.P, self.c
        S = x.shape[0]
        w4 = self.w4_prefill        # (the mode is fixed at construction, as every mode of the decoder is)
        f8 = (self.f8_prefill or w4) and S > 16 and pos_dev is None
        for i in range(c["num_layers"]):
            l = f"model.layers.{i}."
            qkv_names = [l + "self_attn.q_proj", l + "self_attn.k_proj", l + "self_attn.v_proj"]
            gu_names = [l + "mlp.gate_proj", l + "mlp.up_proj"]
            h = ops.rmsnorm(x, P.f32(l + "input_layernorm.weight"), c["rms_eps"])
            if f8:      # fp8 MFMA prefill (config C4): activations quantised per token, weights per output channel, fp32 accumulation
                qkv = ops.linear_f8(*ops.quantize_fp8(h), *P.fp8(qkv_names, stored=l + "self_attn.qkv_proj"))
            else:
                wqkv, _ = P.fused(qkv_names, stored=l + "self_attn.qkv_proj")
                qkv = ops.linear(h, wqkv)
            ops.rope_kv_append_(qkv, self.kc[i], self.vc[i], self.cos, self.sin, self.H, self.Hkv, self.hd, pos0, pos_dev)
            if kv_hook is not None:
                kv_hook(i)
            q = qkv[:, : self.H * self.hd].view(1, S, self.H, self.hd)
            if pos_dev is None:
                n = pos0 + S
                o = ops.attention(q, self.kc[i][:n].unsqueeze(0), self.vc[i][:n].unsqueeze(0), self.hd ** -0.5, causal=True,
                                  window=self.window)
            else:
                o = ops.attention_decode(q, self.kc[i], self.vc[i], pos_dev, self.hd ** -0.5, window=self.window)
            if f8:
                x = ops.linear_f8(*ops.quantize_fp8(o.view(S, self.D)), *P.fp8(l + "self_attn.o_proj"), residual=x)
                h = ops.rmsnorm(x, P.f32(l + "post_attention_layernorm.weight"), c["rms_eps"])
                if w4:      # MXFP4 prefill: e4m3 activations x the packed rows the decode step streams (vg_gemm_w4a8)
                    a = ops.linear_w4a8(*ops.quantize_fp8(h), P.fp4(gu_names, stored=l + "mlp.gate_up_proj"), glu=True)
                    x = ops.linear_w4a8(*ops.quantize_fp8(a), P.fp4(l + "mlp.down_proj"), residual=x)
                    continue
                a = ops.linear_f8(*ops.quantize_fp8(h), *P.fp8(gu_names, stored=l + "mlp.gate_up_proj"), glu=True)
                x = ops.linear_f8(*ops.quantize_fp8(a), *P.fp8(l + "mlp.down_proj"), residual=x)
                continue
            x = ops.linear(o.view(S, self.D), P.w(l + "self_attn.o_proj"), residual=x)
            h = ops.rmsnorm(x, P.f32(l + "post_attention_layernorm.weight"), c["rms_eps"])
            if w4:
                # MXFP4 prefill off the tile path (S <= 16, or a device-side position): the MLP on the decode step's B-row GEMV, 16 rows at a time
                wgu4, wd4 = P.fp4(gu_names, stored=l + "mlp.gate_up_proj"), P.fp4(l + "mlp.down_proj")
                y = torch.empty_like(x)
                for r in range(0, S, 16):
                    a = ops.decode_gemv_w4_rows(h[r:r + 16], wgu4, glu=True)
                    ops.decode_gemv_w4_rows(a, wd4, residual=x[r:r + 16], out=y[r:r + 16])
                x = y
                continue
            wgu, _ = P.fused(gu_names, stored=l + "mlp.gate_up_proj")
            # gate|up in one GEMM; for the decode step the SwiGLU runs in that GEMV's epilogue (ops.linear(glu=True))
            x = ops.linear(ops.linear(h, wgu, glu=True), P.w(l + "mlp.down_proj"), residual=x)
        return ops.rmsnorm(x, P.f32("model.norm.weight"), c["rms_eps"])

    def _layers_decode(self, x, rope_row=True):
        """the same stack for ONE new row at position *pos_dev, on the fused decode kernels: 5 launches per layer
        (norm+qkv[+rope+append], [rope+append+]attention+merge, o+residual, norm+gate|up+SwiGLU, down+residual) instead of 9."""
        P, c = self.P, self.c
        if self.attn_ws is None:
            self.attn_ws = ops.decode_attention_workspace(self.H, self.Hkv, self.hd, self.max_len, x.device)
        if self.chain_roles:
            if self.chain_flags is None:
                self.chain_flags = ops.decode_layer_flags(c["num_layers"], x.device)
                self.chain_err = torch.zeros((), dtype=torch.int32, device=x.device)
            self.chain_err.add_(self.chain_flags[:, 1].sum())      # the previous token's gave-up words survive the memset below (generate() checks)
            self.chain_flags.zero_()          # one memset per token: every layer's arrival stripes and go flags
        pr = self.proj
        if self.rope_path and rope_row:
            ops.decode_advance_(self.pos_dev, 0, rope=(self.cos, self.sin, self.rope_cs))      # the cos / sin row of *pos_dev, once per token (decode_step_begin does it inside a captured step)
        for i in range(c["num_layers"]):
            l = f"model.layers.{i}."
            if self.rope_path:
                # norm -> q|k|v -> RoPE -> append in one launch; the attention starts on its K / V loads (4 launches per layer + the MLP's 2)
                qkv_rope, attn2, kc, vc = ((ops.decode_qkv_rope_kv8, ops.decode_attention2_kv8, self.kc8, self.vc8) if self.kv8 else
                                           (ops.decode_qkv_rope, ops.decode_attention2, self.kc, self.vc))
                q = qkv_rope(x, *pr.operands(P, "qkv", l), P.f32(l + "input_layernorm.weight"), c["rms_eps"], kc[i], vc[i],
                             self.rope_cs, self.pos_dev, self.H, self.Hkv, self.hd)
                o = attn2(q, kc[i], vc[i], self.H, self.Hkv, self.hd, self.pos_dev, self.hd ** -0.5, self.attn_ws,
                          window=self.window, keys_per_wg=self.kpw2)
                x = pr.run("o", False, P, l, o, residual=x)
            else:
                qkv = pr.run("qkv", False, P, l, x, norm_w=P.f32(l + "input_layernorm.weight"), eps=c["rms_eps"])
                if self.chain_roles:
                    # r03: attention, o_proj and (bf16 Llama widths) the MLP as roles of ONE launch whose GEMV workgroups fetch their weight
                    # rows while the producer role still runs (vg_decode_layer) — bit-identical to the separate launches below
                    w_o = P.w(l + "self_attn.o_proj")
                    mlp = None
                    if self.chain_roles == 3 and not (self.w8 or self.w4):     # the chained MLP role streams bf16 weights only
                        wgu, _ = P.fused([l + "mlp.gate_proj", l + "mlp.up_proj"], stored=l + "mlp.gate_up_proj")
                        mlp = (P.f32(l + "post_attention_layernorm.weight"), c["rms_eps"], wgu, P.w(l + "mlp.down_proj"))
                    x = ops.decode_layer(qkv, self.kc[i], self.vc[i], self.cos, self.sin, self.H, self.Hkv, self.hd, self.pos_dev, self.hd ** -0.5,
                                         self.attn_ws, self.chain_flags[i], w_o, x, window=self.window, mlp=mlp)
                    if mlp is not None:
                        continue
                else:
                    attn, kc, vc = (ops.decode_attention_kv8, self.kc8, self.vc8) if self.kv8 else (ops.decode_attention, self.kc, self.vc)
                    o = attn(qkv, kc[i], vc[i], self.cos, self.sin, self.H, self.Hkv, self.hd,
                             self.pos_dev, self.hd ** -0.5, self.attn_ws, window=self.window, keys_per_wg=self.kpw)
                    x = pr.run("o", False, P, l, o, residual=x)
            # the MLP (81 % of a layer's bytes) in the decode weights' format — the attention projections stay bf16: at K = 4096 an fp8 row is
            # a single batch of loads per lane and the per-row reduction eats the gain (10.4 vs 9.1 us measured)
            a, x = pr.mlp(False, P, l, x, c["rms_eps"])
        return ops.rmsnorm(x, P.f32("model.norm.weight"), c["rms_eps"])

    def forward(self, x):
        """eager: x [S,D] new tokens appended at self.pos -> final-normed hidden [S,D] (also kept in hid_all)."""
        S, pos = x.shape[0], self.pos
        assert pos + S <= self.max_len
        self.check_dense(self.c)        # (the decoder's own cfg dict edited in place after a drop)
        if self.kv8 and pos > self.staged:
            # rows [staged, pos) came from decode steps, which append to the e4m3 cache only: the staging takes what that cache holds
            for i in range(self.c["num_layers"]):
                self.kc[i][self.staged:pos].copy_(ops.kv_dequantize(self.kc8[i][self.staged:pos]))
                self.vc[i][self.staged:pos].copy_(ops.kv_dequantize(self.vc8[i][self.staged:pos]))
        h = self._layers(x, pos, None)
        if self.kv8:
            for i in range(self.c["num_layers"]):      # the rows this prefill wrote, [pos, pos + S), into the cache the decode step reads
                ops.kv_quantize_(self.kc[i][pos:pos + S], self.kc8[i][pos:pos + S])
                ops.kv_quantize_(self.vc[i][pos:pos + S], self.vc8[i][pos:pos + S])
            self.staged = pos + S
        self.hid_all[pos:pos + S].copy_(h)
        self.pos = pos + S
        self.pos_dev.fill_(self.pos)
        return h

    def forward_sharded(self, x, comm):
        """sequence-parallel prefill over comm.world ranks (every rank holds the whole prompt x [S,D] and the whole model):
        rank r runs rows [r*m, (r+1)*m) (m = ceil(S/world)) through every layer; per layer the new K/V rows are all-gathered
        straight into every rank's KV cache (S/world x 2 x Hkv x hd elements per rank: ~0.9 MB at S = 1697, world = 8) and a
        row attends causally to the keys [0, its position].  The projections of a row do not depend on the other rows, so the
        prefill costs 1/world per rank (plus one weight pass) instead of a whole one on every rank; the final-norm rows are
        all-gathered at the end (the replicated decode continues from the last one)."""
        c = self.c
        if self.kv8:
            raise ValueError("kv_cache = 'fp8' / 'fp8_rope' has no sequence-parallel prefill (forward_sharded): run the model on one GPU, or keep "
                             "kv_cache = 'bf16'")
        S, W, r = x.shape[0], comm.world, comm.rank
        m = -(-S // W)
        a = min(r * m, S)
        n = max(min(m, S - a), 0)                       # this rank's rows [a, a+n)
        assert self.pos == 0 and W * m <= self.max_len
        send = torch.zeros(m, 2, self.Hkv, self.hd, dtype=x.dtype, device=x.device)
        recv = torch.empty(W * m, 2, self.Hkv, self.hd, dtype=x.dtype, device=x.device)

        def gather(i):
            if n:
                send[:n, 0].copy_(self.kc[i][a:a + n])
                send[:n, 1].copy_(self.vc[i][a:a + n])
            comm.all_gather_into(recv, send)
            self.kc[i][:W * m].copy_(recv[:, 0])        # rows >= S are padding: never read, overwritten by the decode appends
            self.vc[i][:W * m].copy_(recv[:, 1])

        hsend = torch.zeros(m, self.D, dtype=x.dtype, device=x.device)
        if n:
            hsend[:n].copy_(self._layers(x[a:a + n].contiguous(), a, None, kv_hook=gather))   # the same stack as forward(), bf16 or fp8 GEMMs
        else:
            for i in range(c["num_layers"]):      # a rank without rows still takes part in every gather
                gather(i)
        # every rank gets every final-norm row: the decode continues from the last one, and [SEG] tokens that sit INSIDE the prompt
        # (multi-turn) take their hidden state from prompt rows (S x D elements once per clip: 14 MB at S = 1697)
        hrecv = torch.empty(W * m, self.D, dtype=x.dtype, device=x.device)
        comm.all_gather_into(hrecv, hsend)
        self.hid_all[:W * m].copy_(hrecv)
        last = self.hid_all[S - 1:S].clone()
        self.pos = S
        self.pos_dev.fill_(S)
        return last

    def next_token(self, hidden_row):
        """lm_head + argmax (or, sampling, the warpers + the draw of step *step_dev) of one final-norm row -> tok_dev (device int64[1])."""
        if hidden_row.shape[0] == 1:
            logits = self.proj.lm_head(False, self.P, hidden_row)
        else:       # a block of rows (the prefill's): the GEMM, whatever the decode mode
            logits = ops.linear(hidden_row, self.P.w("lm_head"), out_dtype=torch.float32)
        if self.sampling is not None:
            ops.sample_partial(logits[-1], self.samp_params, self.step_dev, tok=self.tok_dev, fast_ws=self.samp_ws if self.samp_fast else None)
        else:
            ops.argmax(logits.view(1, -1), out=self.tok_dev)
        if self.scores_on:
            self._record_scores(logits[-1:], tok=self.tok_dev)

    def _decode_step(self):
        """static step: consume tok_dev at position *pos_dev, emit the next token into tok_dev, advance pos_dev."""
        if not (self.fused_decode and self.P.device.type == "cuda"):
            x = ops.embed(self.tok_dev, self.P.t("model.embed_tokens.weight"))
            h = self._layers_decode(x) if self.fused_decode else self._layers(x, 0, self.pos_dev)
            ops.store_row_(h, self.hid_all, self.pos_dev)
            self.next_token(h)
            self.advance(1)
            return
        # head and tail of the step as one launch each (embed + cos / sin row; token decode + row store + bookkeeping): 3 launches where there were 8
        x = ops.decode_step_begin(self.tok_dev, self.P.t("model.embed_tokens.weight"), self.pos_dev,
                                  rope=(self.cos, self.sin, self.rope_cs) if self.rope_path else None)
        h = self._layers_decode(x, rope_row=False)
        logits = self.proj.lm_head(False, self.P, h)
        if self.sampling is not None:
            ops.sample_partial(logits.view(-1), self.samp_params, self.step_dev, acc=self.amax_acc,     # the same hand-off as argmax_partial
                               fast_ws=self.samp_ws if self.samp_fast else None)
        else:
            ops.argmax_partial(logits.view(-1), self.amax_acc)
        if self.scores_on:
            # *step_dev still names the token being emitted and amax_acc holds the model's own pick (decode_step_end forces, counts and clears)
            self._record_scores(logits.view(1, -1), acc=self.amax_acc)
        ops.decode_step_end(self.amax_acc, self.tok_dev, self.pos_dev, self.step_dev, h, self.hid_all, self.forced, self.hist, self.raw)

    def advance(self, inc):
        """the host's part of HF generate()'s loop, on the device: force / record the token in tok_dev, count the step, move the position"""
        ops.decode_advance_(self.pos_dev, inc, self.tok_dev, self.step_dev, self.forced, self.hist, self.raw)

    def set_forced(self, table):
        """{step: token id} applied to the emitted tokens on the device (step 0 = the token the prefill emits); None / {} = no forcing"""
        f = torch.full((self.HIST,), -1, dtype=torch.int64)
        for k, v in (table or {}).items():
            if 0 <= int(k) < self.HIST:
                f[int(k)] = int(v)
        self.forced.copy_(f.to(self.forced.device))

    def decode_step(self):
        assert self.pos + 1 <= self.max_len
        # long caches: two 64-key blocks per decode-attention workgroup (half the partials to publish, arrive and merge: the merge of a C2 prompt's
        # 54 splits took two passes); a launch parameter, so each setting has its own captured graph.  VG_DEC_KPW_MIN = first position that uses it
        self.kpw = 128 if (self.pos >= self.kpw_min and not self.rope_path) else 0
        if self.kv8:
            self.staged = min(self.staged, self.pos)       # row pos is appended to the e4m3 cache only
        # the route (greedy / fast / general sampler) is part of the captured launches; T, k, p and the seed are not
        key = self.kpw if self.sampling is None else (self.kpw, "sample_fast" if self.samp_fast else "sample")
        if self.scores_on:
            key = (key if isinstance(key, tuple) else (key,)) + ("scores",)
        self.graph = self.graphs.get(key)
        if not self.use_graph:
            self._decode_step()
        else:
            if self.graph is None:
                self.graph = self.graphs[key] = capture_step(self._decode_step, (self.tok_dev, self.pos_dev, self.step_dev))
            self.graph.replay()
        self.pos += 1


def capture_step(step, state):
    """step() captured into a HIP graph that is returned ready to replay: one eager step first (lazy weight packing, kernel attribute setup), then
    the state tensors (token, position, step counter) are put back, the step is captured, and they are put back again"""
    snap = [t.clone() for t in state]
    step()
    torch.cuda.synchronize()
    for t, v in zip(state, snap):
        t.copy_(v)
    g = torch.cuda.CUDAGraph()
    # thread-local capture mode: in multi-GPU runs the RCCL watchdog thread of torch.distributed polls events of finished collectives; under
    # the default (global) mode such a call from another thread can invalidate the capture (ops.graph_capture, which also holds the cyclic GC off)
    with ops.graph_capture(g):
        step()
    for t, v in zip(state, snap):
        t.copy_(v)
    return g


class RowsDecode:
    """The batched decode step of several prompts that share the prefix rows [0, P) of a LlamaDecoder (prompts.generate_prompts): one
    step consumes one token per row and emits one token per row; row b is bit-identical to the single-row step of prompt b alone.

    Key / value rows below row0 = floor(P / kw) * kw (kw = the attention's keys per workgroup) are read from the decoder's caches; every row b has its
    own zero-filled slot of rows [row0, n_bound) (the straddling block [row0, P) copied in once, then its suffix prefill and its decode rows), its
    own final-norm rows (hid[b], position p at p - row0), token, position, step counter, accumulator, forcing table and sampling parameter block.
    Two forms of the step, as the decoder's single-row step: the rope path (bf16 head_dim 128: q|k|v + RoPE + append, then vg_decode_attention2_rows;
    kw = dec.kpw2) and the decode_attention path (Phi-3-mini width: q|k|v GEMV, then RoPE + append + attention in vg_decode_attention_rows, whose
    rows pick 64 or 128 keys per workgroup on the device from their own position and dec.kpw_min; kw = ATTN_KW).
    The projections are the decoder's table (dec.proj, DecodeProjections) asked with rows=True: the weights and formats of the single-row step.
    The step is captured once per sampling route ("greedy" / "sample_fast" / "sample") into a HIP graph; a new seed or temperature is a copy into
    samp_params.  Rows past the live prompts (bucket padding) and retired rows keep computing into their own slots; their tokens are ignored."""

    ATTN_KW = 128      # the decode_attention path's largest split: row0 a multiple of it keeps 64- and 128-key splits wholly shared or per slot

    def __init__(self, dec, bucket, row0, n_bound):
        self.dec, self.B, self.row0, self.n_bound = dec, bucket, row0, n_bound
        d, dev, dt = dec, dec.P.device, dec.P.dtype
        B = bucket
        self.attn_rows = not d.rope_path
        assert row0 % (self.ATTN_KW if self.attn_rows else d.kpw2) == 0
        rows = n_bound - row0
        # the decoder's fp8 K/V cache: the slots hold e4m3 codes as kc8 / vc8 do, on either form of the step ("fp8": decode_attention
        # rows; "fp8_rope": the rope form)
        self.kv8 = bool(getattr(d, "kv8", False))
        assert not self.kv8 or self.attn_rows == (d.kv8 is True)
        kdt = torch.uint8 if self.kv8 else dt
        self.ks = [torch.zeros(B, rows, d.Hkv, d.hd, dtype=kdt, device=dev) for _ in range(d.c["num_layers"])]
        self.vs = [torch.zeros(B, rows, d.Hkv, d.hd, dtype=kdt, device=dev) for _ in range(d.c["num_layers"])]
        self.hid = torch.zeros(B, rows, d.D, dtype=dt, device=dev)
        self.tok = torch.zeros(B, dtype=torch.int64, device=dev)
        self.pos = torch.zeros(B, dtype=torch.int32, device=dev)
        self.step = torch.zeros(B, dtype=torch.int32, device=dev)
        self.acc = torch.zeros(B, dtype=torch.int64, device=dev)
        self.hist = torch.zeros(B, d.HIST, dtype=torch.int64, device=dev)
        self.raw = torch.zeros(B, d.HIST, dtype=torch.int64, device=dev)
        self.forced = torch.full((B, d.HIST), -1, dtype=torch.int64, device=dev)
        self.rope_cs = torch.zeros(B, d.hd, dtype=torch.float32, device=dev)
        self.samp_params = torch.zeros(B, 6, dtype=torch.int32, device=dev)
        self.samp_ws = None
        if self.attn_rows:
            self.attn_ws = ops.decode_attention_rows_workspace(d.H, d.Hkv, d.hd, n_bound, B, dev)
        else:
            self.attn_ws = ops.decode_attention2_rows_workspace(d.H, d.Hkv, d.hd, n_bound, d.kpw2, B, dev)
        self.route = "greedy"
        self.scores_on, self.score_hist, self.top2_hist, self.score_ws = False, None, None, None      # set_scores
        self.graphs = {}
        self.steps = 0          # replayed (or eager) steps since the object was made: the batched loop's step count
        self.host_pos = [0] * B  # every row's position, known on the host: a step past n_bound is refused before it is launched
        self.start_pos = [0] * B  # the positions the rows were loaded at (load_row / pad_row)

    def set_scores(self, on):
        """LlamaDecoder.set_scores for the B rows: score_hist float32 / top2_hist int64 [B, HIST, 2], one ops.token_scores_rows launch per step"""
        self.scores_on = bool(on)
        if self.scores_on and self.score_hist is None:
            dev = self.dec.P.device
            self.score_hist = torch.zeros(self.B, self.dec.HIST, 2, dtype=torch.float32, device=dev)
            self.top2_hist = torch.zeros(self.B, self.dec.HIST, 2, dtype=torch.int64, device=dev)
            self.score_ws = ops.token_scores_workspace(self.B, dev)

    def load_row(self, b, P, end):
        """row b continues from the decoder's state after prompt b's suffix prefill and first token: its K / V rows [row0, end) and final-norm rows
        [P, end) are copied into slot b; token, position (end), step (1: the prefill's token is step 0) and sampling block from the decoder."""
        d = self.dec
        kc, vc = (d.kc8, d.vc8) if self.kv8 else (d.kc, d.vc)
        for i in range(d.c["num_layers"]):
            self.ks[i][b, :end - self.row0].copy_(kc[i][self.row0:end])
            self.vs[i][b, :end - self.row0].copy_(vc[i][self.row0:end])
        self.hid[b, P - self.row0:end - self.row0].copy_(d.hid_all[P:end])
        self.host_pos[b] = self.start_pos[b] = end
        self.tok[b:b + 1].copy_(d.tok_dev)
        self.pos[b] = end
        self.step[b] = 1
        self.acc[b] = 0
        self.forced[b].fill_(-1)
        if d.sampling is not None:
            self.samp_params[b].copy_(d.samp_params)
        if self.scores_on:      # slot 0: the record the decoder's single-row step left for the prefill's token
            self.score_hist[b, 0].copy_(d.score_hist[0])
            self.top2_hist[b, 0].copy_(d.top2_hist[0])

    def pad_row(self, b, P, like=0):
        """a bucket row without a prompt: position P of its own slot, token 0, row `like`'s sampling block"""
        self.tok[b] = 0
        self.pos[b] = P
        self.host_pos[b] = self.start_pos[b] = P
        self.step[b] = 1
        self.acc[b] = 0
        self.samp_params[b].copy_(self.samp_params[like])

    def _step(self):
        d, P, c = self.dec, self.dec.P, self.dec.c
        pr = d.proj
        x = ops.decode_step_begin_rows(self.tok, P.t("model.embed_tokens.weight"), self.pos,
                                       rope=None if self.attn_rows else (d.cos, d.sin, self.rope_cs))
        for i in range(c["num_layers"]):
            l = f"model.layers.{i}."
            if self.attn_rows:
                qkv = pr.run("qkv", True, P, l, x, norm_w=P.f32(l + "input_layernorm.weight"), eps=c["rms_eps"])
                attn, kc, vc = (ops.decode_attention_rows_kv8, d.kc8, d.vc8) if self.kv8 else (ops.decode_attention_rows, d.kc, d.vc)
                o = attn(qkv, kc[i], vc[i], self.ks[i], self.vs[i], self.row0, d.cos, d.sin, d.H, d.Hkv, d.hd, self.pos,
                         self.n_bound, d.hd ** -0.5, self.attn_ws, window=d.window, kpw_min=d.kpw_min)
            else:
                qkv_rope, attn2, kc, vc = ((ops.decode_qkv_rope_rows_kv8, ops.decode_attention2_rows_kv8, d.kc8, d.vc8) if self.kv8 else
                                           (ops.decode_qkv_rope_rows, ops.decode_attention2_rows, d.kc, d.vc))
                q = qkv_rope(x, *pr.operands(P, "qkv", l), P.f32(l + "input_layernorm.weight"), c["rms_eps"], self.ks[i], self.vs[i],
                             self.row0, self.rope_cs, self.pos, d.H, d.Hkv, d.hd)
                o = attn2(q, kc[i], vc[i], self.ks[i], self.vs[i], self.row0, d.H, d.Hkv, d.hd, self.pos, self.n_bound,
                          d.hd ** -0.5, self.attn_ws, window=d.window, keys_per_wg=d.kpw2)
            x = pr.run("o", True, P, l, o, residual=x)
            a, x = pr.mlp(True, P, l, x, c["rms_eps"])
        h = ops.rmsnorm(x, P.f32("model.norm.weight"), c["rms_eps"])
        logits = pr.lm_head(True, P, h)
        if self.route == "greedy":
            ops.argmax_partial_rows(logits, self.acc)
        else:
            # vg_sample for the B rows in one launch: every row its own parameter block, step counter, accumulator and (fast route) workspace
            ops.sample_partial_rows(logits, self.samp_params, self.step, acc=self.acc, fast_ws=self.samp_ws if self.route == "sample_fast" else None)
        if self.scores_on:
            # one launch for the B rows: step[b] still names the token row b emits, acc[b] holds the row's own pick
            ops.token_scores_rows(logits, self.step, self.score_hist, self.top2_hist, acc=self.acc, ws=self.score_ws)
        ops.decode_step_end_rows(self.acc, self.tok, self.pos, self.step, h, self.hid, forced=self.forced, hist=self.hist, raw=self.raw,
                                 hid_row0=self.row0)

    def set_positions(self, pos):
        """rows' positions (host list, each in [row0, n_bound)): written to the device and tracked on the host"""
        assert all(self.row0 <= p < self.n_bound for p in pos)
        self.host_pos = list(pos)
        self.pos.copy_(torch.tensor(pos, dtype=torch.int32))

    def decode_step(self):
        if max(self.host_pos) >= self.n_bound:
            raise ValueError(f"RowsDecode: a row at position {max(self.host_pos)} is past the slots' bound {self.n_bound}")
        if self.route != "greedy" and self.samp_ws is None:
            self.samp_ws = ops.sample_workspace_rows(self.B, self.dec.P.device)
        self.steps += 1
        self.host_pos = [p + 1 for p in self.host_pos]
        if not self.dec.use_graph:
            self._step()
            return
        key = (self.route, "scores") if self.scores_on else self.route
        g = self.graphs.get(key)
        if g is None:
            g = self.graphs[key] = capture_step(self._step, (self.tok, self.pos, self.step))
        g.replay()

    def rows_of(self, b, P, rows):
        """final-norm rows of prompt b at sequence rows `rows`: below P from the decoder (the shared prefix), from P on from slot b"""
        d = self.dec
        return torch.stack([d.hid_all[r] if r < P else self.hid[b, r - self.row0] for r in rows])

def splice(params, input_ids, visual):
    """prepare_inputs_labels_for_multimodal for one sample with one run of <image> placeholders —
    R/model/videogpt_plus/model/arch.py:271-371,453-467.  input_ids [L] (host, with -200) -> embeds [S,D]."""
    ids = input_ids
    pos = (ids == IMAGE_TOKEN_INDEX).nonzero().flatten()
    table = params.t("model.embed_tokens.weight")
    dev = params.device
    if pos.numel() == 0:
        return ops.embed(ids.to(dev), table)
    s, e = int(pos[0]), int(pos[-1])
    parts = [ops.embed(ids[:s].to(dev), table), visual]
    if e + 1 < ids.numel():
        parts.append(ops.embed(ids[e + 1:].to(dev), table))
    return torch.cat(parts, dim=0).contiguous()


def stage_mark(stages, name):
    """diagnostics (bench.py's per-stage split): when `stages` is a list, wait for the device and append (name, host time)."""
    if stages is not None:
        import time
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        stages.append((name, time.perf_counter()))


def generate(params, cfg, towers, images, context_images, input_ids, max_new_tokens, eos_token_id=None, visual=None,
             token_hook=None, after_prefill=None, comm=None, trace=None, stages=None, sampling=None):
    """Steps A–D of VideoGLaMM_SAM2.inference_* (R/model/VideoGLaMM.py:609-655 / 781-831) with encode-once +
    KV-cache scheduling.  The hidden state the reference gathers for a [SEG] at output position p is the
    final-norm state of position p-1 = the row that produced the token, captured here as it is
    emitted.  token_hook(step, token_id) -> token_id | None: called with every emitted token AFTER the full lm_head + argmax (the place of a
    logits processor in HF generate()); a returned id replaces the token (teacher forcing in tests; synth.forced_tokens_hook for the synthetic-weight
    benchmark, whose random weights never emit [SEG] — no work is skipped).
    trace: optional dict; trace["argmax"] receives the model's own argmax of every step (before any forcing).  A caller that puts
    trace["scores"] = True gets it replaced by {"logprob": float32 [G], "margin": float32 [G], "top2": int64 [G, 2]} (host numpy, G = generated
    tokens): log_softmax of the raw logits at the model's own pick, the top-2 margin and the top-2 indices of every step.
    eos_token_id: one id or several (HF generate() stops on any id of generation_config.eos_token_id).
    sampling: None = greedy; dict(T=, k=, p=, seed=) = HF's do_sample decoding (Temperature -> TopK -> TopP, then a draw) on the device,
    token j drawn with the uniform of Philox counter j; trace["argmax"] then holds the drawn ids before forcing.
    input_ids: host int64 [L] -> (output_ids host int64 [L+G], pred_embeddings device [N,256])."""
    seg_idx = cfg["seg_token_idx"]
    eos = set() if eos_token_id is None else ({int(eos_token_id)} if isinstance(eos_token_id, int) else {int(e) for e in eos_token_id})
    stage_mark(stages, "start")
    if visual is None:
        visual = towers.encode(images, context_images, comm)
    stage_mark(stages, "towers")
    x = splice(params, input_ids, visual)
    need = x.shape[0] + max_new_tokens + 1
    dec = getattr(params, "_decoder", None)
    if dec is None or dec.max_len < need:
        dec = LlamaDecoder(params, cfg["llm"], -(-need // 1024) * 1024)
        params._decoder = dec          # KV cache + captured decode graph are reused across clips
    dec.check_dense(cfg["llm"])        # (a kept decoder does not follow the live cfg; after dense_mlp = "drop" a cfg that asks for a dense mode is refused, not ignored)
    dec.reset()
    dec.set_sampling(sampling)
    dec.set_scores(wants_scores(trace))
    if comm is not None and comm.world > 1 and x.shape[0] >= 64 * comm.world and os.environ.get("VG_PREFILL_SHARDED", "0") == "1":
        hidden = dec.forward_sharded(x, comm)   # opt-in sequence-parallel prefill: 1/world of the rows per rank (row chunks of another
        #                                         M take other GEMM routes: bf16 ids may differ from the single-GPU run; default = replicated)
    else:
        hidden = dec.forward(x)[-1:]            # hid_all rows 0..S-1: final-norm states of the spliced prompt
    added = x.shape[0] - input_ids.numel()      # "num_newly_added_tokens" (VideoGLaMM.py:613,786)
    ids = input_ids.tolist()
    if max_new_tokens > 0:
        dec.next_token(hidden)
    stage_mark(stages, "prefill")
    if after_prefill is not None:
        after_prefill()   # e.g. enqueue the (LLM-independent, MFMA-bound) Hiera pass on a side stream so that it
        #                   overlaps the HBM-bound decode loop below
    decode_loop(params, dec, ids, max_new_tokens, eos, token_hook, trace)
    out_ids = torch.tensor(ids, dtype=torch.int64)
    # seg_token_mask = (output_ids[:,1:] == seg) left-padded by `added` (VideoGLaMM.py:630-633,803-806):
    # the row picked for a [SEG] at output position j is j-1+added, i.e. the state that emitted it
    rows = [j - 1 + added for j in range(1, len(ids)) if ids[j] == seg_idx]
    if not rows:
        stage_mark(stages, "decode")
        return out_ids, torch.empty(0, 256, dtype=params.dtype, device=params.device)
    h = dec.hid_all[torch.tensor(rows, device=params.device)]
    fc = "model.text_hidden_fcs.0."
    h = ops.linear(h, params.w(fc + "0"), params.b(fc + "0"), act=ops.ACT_RELU)
    emb = ops.linear(h, params.w(fc + "2"), params.b(fc + "2"))
    stage_mark(stages, "decode")
    return out_ids, emb


def wants_scores(trace):
    """True for a trace dictionary whose caller put trace["scores"] = True (generate() replaces it by the records)"""
    return trace is not None and trace.get("scores") is True


def read_scores(score_hist, top2_hist, G):
    """the records of the first G emitted tokens of one row (score_hist float32 [HIST, 2], top2_hist int64 [HIST, 2]), read back once ->
    {"logprob": float32 [G], "margin": float32 [G], "top2": int64 [G, 2]} as host numpy arrays"""
    import numpy as np
    if G <= 0:
        return {"logprob": np.zeros(0, np.float32), "margin": np.zeros(0, np.float32), "top2": np.zeros((0, 2), np.int64)}
    sc, t2 = score_hist[:G].cpu().numpy(), top2_hist[:G].cpu().numpy()
    return {"logprob": sc[:, 0].copy(), "margin": sc[:, 1].copy(), "top2": t2.copy()}


def decode_loop(params, dec, ids, max_new_tokens, eos, token_hook=None, trace=None):
    """generate()'s token loop from the token the prefill emitted (dec.next_token already enqueued): appends the emitted ids to the host list
    `ids` until an id of `eos` or max_new_tokens; dec's hid_all then holds the final-norm row of every decoded position.  A trace that asks for
    scores (wants_scores; the caller has switched dec.set_scores on before the first token) receives the records of the emitted tokens."""
    n_prompt = len(ids)
    # The loop.  Forcing / recording / the position bump can happen on the device (LlamaDecoder.advance), so with no Python hook in the way step k + 1
    # can be enqueued BEFORE token k is read back (VG_DECODE_AHEAD=1: tokens return on a side stream behind per-step events; the step launched while
    # an EOS token was in flight is wasted — it writes cache rows past the end that nobody reads).  Built for VERDICT r05 item 1(c) and measured r06 on C2
    # (tools/lab/r06_c2_ab.sh, same box): the synchronous hand-over costs ~16 us per token in the serial decode stage (2.98 ms wall vs 2.966 ms of graph
    # time), and the run-ahead loop's events + side-stream copies make every replayed step ~0.17 ms LONGER (3.13 vs 2.97 ms per token; clip 252.6 vs
    # 248.2 ms) — so the default is the synchronous loop; the opt-in stays for runtimes where the hand-over is the larger term.
    # token_hook: a dict-carrying hook (synth.forced_tokens_hook: hook.forced_table = {step: id}) can be applied on the device; any other callable
    # is opaque Python and always keeps the synchronous hand-over.
    table = getattr(token_hook, "forced_table", None) if token_hook is not None else {}
    ahead = (table is not None and os.environ.get("VG_DECODE_AHEAD", "0") == "1" and max_new_tokens <= dec.HIST and params.device.type == "cuda"
             and dec.use_graph)
    if max_new_tokens > 0:
        dec.set_forced(table if ahead else None)
        dec.step_dev.zero_()
        dec.advance(0)                       # token 0 (emitted by the prefill): forced / recorded; the position stays
    if ahead:
        # tokens come back on a side stream that waits only for the step that emitted them (an event per step), never for the step enqueued after it
        main = torch.cuda.current_stream()
        rb = dec.__dict__.setdefault("_rb_stream", torch.cuda.Stream())
        host = dec.__dict__.setdefault("_rb_host", torch.zeros(2, dec.HIST, dtype=torch.int64).pin_memory())
        evs = [torch.cuda.Event()]           # evs[j]: token j is in hist[j] / raw[j]
        evs[0].record(main)
        known = 0
        while max_new_tokens > 0:
            if len(evs) < max_new_tokens:    # run ahead by one: step len(evs) - 1 consumes token len(evs) - 1 and emits token len(evs)
                dec.decode_step()
                evs.append(torch.cuda.Event())
                evs[-1].record(main)
                upto = len(evs) - 1          # read what the steps BEFORE this one emitted
            else:
                upto = len(evs)              # nothing left to launch: read the last token too
            with torch.cuda.stream(rb):
                rb.wait_event(evs[upto - 1])
                host[0, known:upto].copy_(dec.hist[known:upto], non_blocking=True)
                if trace is not None:
                    host[1, known:upto].copy_(dec.raw[known:upto], non_blocking=True)
            rb.synchronize()
            stop = False
            for j in range(known, upto):
                if trace is not None:
                    trace.setdefault("argmax", []).append(int(host[1, j]))
                ids.append(int(host[0, j]))
                known += 1
                if ids[-1] in eos or known == max_new_tokens:
                    stop = True
                    break
            if stop:
                break
    else:
        for step in range(max_new_tokens):
            nxt = int(dec.tok_dev[0])
            if trace is not None:
                trace.setdefault("argmax", []).append(nxt)
            if token_hook is not None:
                repl = token_hook(step, nxt)
                if repl is not None and int(repl) != nxt:
                    nxt = int(repl)
                    dec.tok_dev.fill_(nxt)
            ids.append(nxt)
            if nxt in eos or step == max_new_tokens - 1:
                break
            dec.decode_step()
    if wants_scores(trace):      # one read after the loop, cut to the tokens this prompt emitted
        trace["scores"] = read_scores(dec.score_hist, dec.top2_hist, len(ids) - n_prompt)
    if dec.chain_roles and dec.chain_flags is not None and int(dec.chain_err) + int(dec.chain_flags[:, 1].sum()):
        # VG_DECODE_CHAIN: a workgroup of a chained layer launch stopped waiting for its producer role (bounded wait) — the ids above are not to be trusted
        raise ops._lib.VGKernelError("vg_decode_layer: a device-side wait gave up (flags[1] set); rerun with VG_DECODE_CHAIN=0")
