/*
 * vg_kernels.h — C ABI of libvgkernels.so, the hand-written gfx950 (MI355X / CDNA4) kernel
 * library behind the VideoGLaMM inference hot path.
 *
 * Conventions:
 *   - plain pointers and sizes only; every buffer (inputs, outputs, workspace) is owned by the
 *     caller and lives in device memory; no hidden allocation, no implicit synchronisation;
 *   - every entry point is stateless, re-entrant and stream-ordered on the hipStream_t passed last;
 *   - return value 0 = VG_OK, negative = error code; vg_last_error() gives a thread-local message;
 *   - activations / weights are VG_F32 or VG_BF16 (raw uint16 storage), accumulation is always fp32;
 *     bias / norm-weight / LayerScale vectors are always fp32;
 *   - tensors are token-major ("channels last"): [tokens, channels] with channels contiguous.
 *
 * R/ = the reference tree /root/reference/VideoGLaMM/. The reference has no native boundary on this
 * path (its only native file, sam2/csrc/connected_components.cu, is dead code on it —
 * R/model/segment_anything_2/sam2/sam2_video_predictor.py:971-975); each entry point below therefore
 * cites the PyTorch call site(s) whose arithmetic it replaces.
 */
#ifndef VG_KERNELS_H
#define VG_KERNELS_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vg_stream_t; /* hipStream_t */

#define VG_F32 0
#define VG_BF16 1

#define VG_OK 0
#define VG_ERR_ARG (-1)
#define VG_ERR_LAUNCH (-2)
#define VG_ERR_UNSUPPORTED (-3)

#define VG_ACT_NONE 0
#define VG_ACT_GELU 1       /* exact erf GELU: nn.GELU() */
#define VG_ACT_QUICK_GELU 2 /* x*sigmoid(1.702x): HF CLIP "quick_gelu" */
#define VG_ACT_RELU 3
#define VG_ACT_SILU 4
#define VG_ACT_SIGMOID 5

int vg_version(void);
const char* vg_last_error(void);
/* Binds nothing; checks that `device` is a gfx950 part. Returns CU count (>0) or a negative code. */
int vg_init(int device);
/* Node census of a captured HIP graph (hipGraph_t): counts[0] = kernel nodes, counts[1] = memcpy nodes, counts[2] = every other node.
 * Measurement aid for the graph-replayed loops (the SAM2 propagation the reference runs as Python calls per frame,
 * R/model/segment_anything_2/sam2/sam2_video_predictor.py:744-827; the decode step): launches per replay, read off the graph itself. */
int vg_graph_node_counts(void* graph, int64_t* counts);

/* ---- dense contraction (MFMA) ------------------------------------------------------------------
 * C[b] = ((act(A[b] @ W[b]^T + bias)) * gamma) + R[b]      A:[M,K] lda, W:[N,K] ldw, C:[M,N] ldc
 * Replaces every nn.Linear / 1x1 conv / im2col'd conv on the path, e.g.
 *   R/model/videogpt_plus/model/internvideo/internvideo2.py:193,207,257-261 (qkv/proj/fc1/fc2 + LayerScale :283-284),
 *   R/model/segment_anything_2/sam2/modeling/backbones/hieradet.py:56,82 ; sam2_utils.py:126-131 (MLP),
 *   R/model/segment_anything_2/sam2/modeling/sam/transformer.py:238-258 (q/k/v/out proj),
 *   R/model/segment_anything_2/sam2/modeling/sam/mask_decoder.py:227-234 (hypernetwork product, batched),
 *   HF LlamaAttention/LlamaMLP projections and lm_head (R/model/videogpt_plus/model/language_model/llama3_1.py:63-75).
 * in_dtype applies to A and W; out_dtype to C and R. K must be a multiple of 8 (bf16) / 4 (f32) and
 * lda/ldw multiples of the same; M, N arbitrary. batch>1 uses element strides sA/sW/sC/sR (sW may be 0).
 */
int vg_gemm(const void* A, int64_t lda, int64_t sA, const void* W, int64_t ldw, int64_t sW,
            void* C, int64_t ldc, int64_t sC, const float* bias, const float* gamma,
            const void* R, int64_t ldr, int64_t sR, int M, int N, int K, int batch,
            int in_dtype, int out_dtype, int act, int a_op, vg_stream_t stream);
/* a_op = 1: W holds 2N rows, gate rows then up rows; C[:, n] = silu(A·W[n] + b[n]) * (A·W[N+n] + b[N+n]) —
 * HF LlamaMLP act(gate_proj(x)) * up_proj(x) with the SwiGLU done in the epilogue (gate / up / act rounded to the
 * output dtype like the separate modules do).  M > 16 additionally needs 16-byte aligned C rows, no R / gamma / act. */

/* Short-row contraction with a row-wise producer and a column-pair consumer in the same launch (bf16, K in {64, 128, 192, 256}, N % 64 == 0):
 *   C = act(pro(A) @ W^T + bias) [axial RoPE] [+ R]
 *   pro: LayerNorm over the K columns (ln_w / ln_b / ln_eps; statistics in fp32, result rounded to bf16 — vg_layernorm followed by vg_gemm), or
 *        A + A2 with A2 [a2_rows, K] repeated over blocks of a2_rows rows (rounded to bf16 — vg_axpby followed by vg_gemm), or nothing (NULLs);
 *   RoPE (rope_cos != NULL): vg_rope_axial_heads on the bf16-rounded product's first rope_cols columns (heads of rope_ch channels), rows
 *        [rope_r0, rope_r1) of every block of rows_per_block rows, token = (row - rope_r0) % rope_grid; no activation / residual with it.
 *   a_block_stride != 0: A is a strided [B, rows_per_block, K] view — row m at (m / rows_per_block) * a_block_stride + (m % rows_per_block) * lda.
 * Replaces, per launch, the module sequences norm1 -> self_attn.{q,k,v}_proj -> apply_rotary_enc, norm2 -> cross_attn_image.q_proj -> rotary,
 * (memory + memory_pos) -> cross_attn_image.k_proj -> rotary with num_k_exclude_rope, norm3 -> linear1 -> ReLU of
 * R/model/segment_anything_2/sam2/modeling/memory_attention.py:60-99 + sam/transformer.py:289-327, and norm -> pwconv1 -> GELU of
 * memory_encoder.py:96-118.  The fp32 parity mode runs the separate entry points. */
int vg_gemm_rows(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, const float* bias, const void* R, int64_t ldr,
                 int64_t M, int N, int K, int act, const float* ln_w, const float* ln_b, float ln_eps, const void* A2, int64_t lda2,
                 int a2_rows, const float* rope_cos, const float* rope_sin, int rope_cols, int rope_ch, int rows_per_block, int64_t a_block_stride,
                 int rope_r0, int rope_r1, int rope_grid, int dtype, vg_stream_t stream);

/* A whole pre-norm MLP block on narrow rows in one launch (bf16; C in {144, 288}: Hiera stages 1 and 2; H % 32 == 0):
 *   y = x + W2 @ gelu(W1 @ LayerNorm(x) + b1) + b2        W1: [H, C] contiguous rows, W2: [C, H] contiguous rows, exact-erf GELU
 * — x = x + self.mlp(self.norm2(x)) of R/model/segment_anything_2/sam2/modeling/backbones/hieradet.py:160-168 (MLP: sam2_utils.py:108-132).
 * The LayerNorm output and the hidden activation are rounded to bf16 like the separate launches' tensors; they never leave the CU.
 * vg_mlp_rows_supported(C, H) != 0: this (C, H) has an instantiation; the fp32 parity mode runs vg_layernorm + vg_gemm x 2. */
int vg_mlp_rows_supported(int C, int H);
int vg_mlp_rows(const void* x, int64_t ldx, void* y, int64_t ldy, const float* ln_w, const float* ln_b, float eps, const void* w1,
                const float* b1, const void* w2, const float* b2, int64_t M, int C, int H, int dtype, vg_stream_t stream);

/* The same contraction with Hiera's window_partition / window_unpartition (backbones/utils.py:16-38,41-60, called from
 * hieradet.py:128-136,147-148) folded into it.  GEMM row m is the WINDOW-order row index (window (b,wy,wx), token (r,c)),
 * M = B*ceil(H/ws)*ceil(W/ws)*ws*ws including the zero padding rows the reference pads with.
 *   mode 1: A is the IMAGE-order tensor [B,H,W,K] (row stride lda); row m is gathered from it (padding rows read
 *           zero_row, K zeros) and C is written in window order — window_partition + qkv projection in one pass.
 *   mode 2: A is window-order; C (row stride ldc) and R (ldr) are IMAGE-order [B,H,W,N]: row m is scattered to its
 *           pixel, padding rows are dropped — proj + window_unpartition + residual add in one pass. */
int vg_gemm_window(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, const float* bias,
                   const float* gamma, const void* R, int64_t ldr, int N, int K, int in_dtype, int out_dtype, int act,
                   int mode, int B, int H, int Wd, int ws, const void* zero_row, vg_stream_t stream);

/* y = act(LayerNorm_K(A rows) @ W^T + bias) — the norm1 -> q|k|v and norm2 -> fc1 pairs of Hiera's MultiScaleBlock at the widths of stages 1 and 2
 * (R/model/segment_anything_2/sam2/modeling/backbones/hieradet.py:117-123, 160-166), the LayerNorm applied to the rows in registers.  Built for the
 * row-register route only: bf16, K in {144, 288}, N a multiple of 16, >= 65536 rows, act none | GELU; VG_ERR_UNSUPPORTED otherwise (the caller then runs
 * vg_layernorm + vg_gemm / vg_gemm_window).  window = 1: rows gathered from an image-order [B,H,W,K] tensor as vg_gemm_window's mode 1 (M is ignored;
 * padding rows stay zero BEHIND the norm, as F.pad of the normalised tensor does); zero_row as in vg_gemm_window. */
int vg_gemm_ln(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, const float* bias,
               const float* ln_w, const float* ln_b, float ln_eps, int64_t M, int N, int K, int act,
               int window, int B, int H, int Wd, int ws, const void* zero_row, int dtype, vg_stream_t stream);


/* ---- attention (flash-style, LDS-staged QK tiles, in-register online softmax) -------------------
 * O[b,i,h,:] = softmax_j(scale * Q[b,i,h,:]·K[b,j,g,:] (+causal mask)) @ V[b,j,g,:],  g = h / (Hq/Hkv)
 * causal = 1: key j visible to query i iff j <= i + (Skv - Sq).  causal = c >= 2: the same with a sliding window of c
 * visible keys, the query's own position included: i + (Skv - Sq) - c < j <= i + (Skv - Sq) (HF Phi-3's sliding_window mask,
 * transformers==4.41.0 modeling_attn_mask_utils._make_causal_mask: c = sliding_window + 1).  causal = -w (w > 0): block-diagonal mask — the
 * sequence is a pack of independent w-token windows (key j visible to query i iff j/w == i/w; Sq == Skv), which lets
 * Hiera's 16- / 64-token windows share 128-query tiles.  D % 8 == 0, D <= 256.
 * Strides are in elements: *_sb batch, *_ss token, *_sh head; the head dim is contiguous.
 * Replaces F.scaled_dot_product_attention / naive softmax(QK^T)V at
 *   R/model/segment_anything_2/sam2/modeling/backbones/hieradet.py:72-76,
 *   R/model/segment_anything_2/sam2/modeling/sam/transformer.py:249-255,316-322,
 *   R/model/videogpt_plus/model/internvideo/internvideo2.py:200-206,
 *   HF CLIPAttention / LlamaAttention (third-party, transformers==4.41.0).
 */
int vg_attention(const void* Q, const void* K, const void* V, void* O, int B, int Hq, int Hkv,
                 int Sq, int Skv, int D, int64_t q_sb, int64_t q_ss, int64_t q_sh, int64_t k_sb,
                 int64_t k_ss, int64_t k_sh, int64_t v_sb, int64_t v_ss, int64_t v_sh, int64_t o_sb,
                 int64_t o_ss, int64_t o_sh, float scale, int causal, int dtype, vg_stream_t stream);

/* Attention inside independent windows: O[w,i,h,:] = softmax_j(scale * Q[w,i,h,:].K[w,j,h,:]) @ V[w,j,h,:], i in [0, wq), j in
 * [0, wtok) — Hiera's MultiScaleAttention on window_partition'ed tokens (R/model/segment_anything_2/sam2/modeling/backbones/
 * hieradet.py:37-83, backbones/utils.py:16-38; wq < wtok: the q-pooled first block of a stage, hieradet.py:64-68).  bf16 only.
 *   wq == wtok == 256, D in {64, 72, 80}: one workgroup per (window, head), the window's K and V staged once (stage 3);
 *   D == 72 and (wq, wtok) in {(16,16), (64,64), (4,16), (16,64)}: one wave per (window, head) on 16x16x32 MFMA tiles.
 * *_sb = window stride, *_ss token stride, *_sh head stride (elements); O may be a strided view as well. */
int vg_window_attention(const void* Q, const void* K, const void* V, void* O, int Bw, int H, int wq, int wtok, int D,
                        int64_t q_sb, int64_t q_ss, int64_t q_sh, int64_t k_sb, int64_t k_ss, int64_t k_sh,
                        int64_t v_sb, int64_t v_ss, int64_t v_sh, int64_t o_sb, int64_t o_ss, int64_t o_sh,
                        float scale, int dtype, vg_stream_t stream);

/* Same contraction with the KV range split over `nsplit` workgroups per (query tile, head) and a merge pass —
 * the decode-step shape (Sq = 1, Skv = thousands: one workgroup per head would walk the whole KV cache
 * serially).  workspace: fp32, >= B*Hq*nsplit*Sq*(D+2) floats, caller-owned.  nsplit = 1 == vg_attention. */
int vg_attention_splitkv(const void* Q, const void* K, const void* V, void* O, int B, int Hq, int Hkv,
                         int Sq, int Skv, int D, int64_t q_sb, int64_t q_ss, int64_t q_sh, int64_t k_sb,
                         int64_t k_ss, int64_t k_sh, int64_t v_sb, int64_t v_ss, int64_t v_sh, int64_t o_sb,
                         int64_t o_ss, int64_t o_sh, float scale, int causal, int dtype, float* workspace,
                         int64_t ws_floats, int nsplit, const int* skv_dev, vg_stream_t stream);
/* skv_dev (may be NULL): when given, the kernel uses Skv = *skv_dev + Sq read from device memory instead of the
 * host value, so one captured decode step can be replayed from a HIP graph as the KV cache grows. */

/* Attention whose VALUES (and output) have DV dims while queries / keys have D (one head group, no mask): SAM2's memory cross-attention
 * with the v-projection moved behind the attention — the reference computes softmax(q k^T) (M Wv^T + b)
 * (R/model/segment_anything_2/sam2/modeling/sam/transformer.py:289-327, memory_attention.py:60-99); softmax rows sum to one, so that equals
 * (softmax(q k^T) M) Wv^T + b: the projection then runs on the 4096 query rows instead of the ~28 000 memory rows and the PV half of the
 * attention works on the memory's own 64 dims.  Built for bf16, D in (128, 256], DV = 64 (VG_ERR_UNSUPPORTED otherwise).  V rows [.., DV], O rows [.., DV];
 * workspace (nsplit > 1): fp32, >= B*H*nsplit*Sq*(DV+2) floats. */
int vg_attention_dv(const void* Q, const void* K, const void* V, void* O, int B, int H, int Sq, int Skv, int D, int DV,
                    int64_t q_sb, int64_t q_ss, int64_t q_sh, int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t v_sb,
                    int64_t v_ss, int64_t v_sh, int64_t o_sb, int64_t o_ss, int64_t o_sh, float scale, int dtype,
                    float* workspace, int64_t ws_floats, int nsplit, vg_stream_t stream);

/* Fused HF rotate-half RoPE + KV-cache append for one decoder layer (HF LlamaAttention.forward: apply_rotary_pos_emb
 * then cache update).  qkv: fused projection output [S, (H+2*Hkv)*D], row stride ld; q rotated in place, rotated k
 * and plain v written to k_cache/v_cache[pos+s] ([max_len,Hkv,D]).  pos = pos_dev ? *pos_dev : pos0. */
int vg_rope_kv_append(void* qkv, int64_t ld, void* k_cache, void* v_cache, const float* cos, const float* sin,
                      int S, int H, int Hkv, int D, int pos0, const int* pos_dev, int dtype, vg_stream_t stream);
/* dst[(*idx_dev + idx_off)*n + i] = src[i]; *p += v — device-indexed bookkeeping for graph-replayed decode. */
int vg_store_row(const void* src, void* dst, int64_t n, const int* idx_dev, int idx_off, int dtype, vg_stream_t stream);
int vg_add_int(int* p, int v, vg_stream_t stream);

/* ---- fused single-token decode step (HF LlamaDecoderLayer.forward at q_len = 1, transformers==4.41.0; called per
 * generated token from R/model/VideoGLaMM.py:616-628 / 789-801 via self.generate) ---------------------------------
 * vg_decode_gemv: y[N] = f(x)[K] . W[N,K]^T (+ R[N]).  norm_w != NULL: f = LlamaRMSNorm(eps) with weight norm_w (fp32
 *   copy of the norm weight) — input_layernorm / post_attention_layernorm fused into the q|k|v and gate|up projections.
 *   glu != 0: W is [2N,K] = gate rows | up rows and y[n] = silu(x.gate_n) * (x.up_n) (LlamaMLP).  Row stride of W = ldw.
 * vg_decode_attention: qkv = fused projection row [(H+2*Hkv)*D] of the new token at position p = *pos_dev.  Applies
 *   rotate-half RoPE (cos/sin tables [max_len, D/2]) to q and k, appends k/v to the caches ([max_len,Hkv,D]) and writes
 *   softmax(q.K[lo..p]^T * scale).V[lo..p] to out [H*D], lo = window > 0 ? max(0, p + 1 - window) : 0 (window = number of
 *   visible positions, the new one included; 0 = the whole cache).  workspace: fp32, vg_decode_attention_ws_floats() floats, must be
 *   zero-filled ONCE by the caller before the first launch (it ends with self-resetting per-head counters).  keys_per_wg: 0 / 64 =
 *   one workgroup per 64 cache positions and KV head; 128 = a hint for long caches (>= ~2048 positions): two 64-key blocks per
 *   workgroup, so half as many partial results are published and merged (same result up to fp32 summation order; honoured for the
 *   bf16 Llama-3 / Phi-3 head shapes, ignored elsewhere). */
int vg_decode_gemv(const void* x, const void* W, int64_t ldw, void* y, const float* norm_w, float eps,
                   const void* R, int N, int K, int glu, int in_dtype, int out_dtype, vg_stream_t stream);
int64_t vg_decode_attention_ws_floats(int H, int Hkv, int D, int max_len);
int vg_decode_attention(const void* qkv, void* k_cache, void* v_cache, const float* cos, const float* sin,
                        void* out, int H, int Hkv, int D, int max_len, int window, float scale, const int* pos_dev,
                        float* workspace, int64_t ws_floats, int keys_per_wg, int dtype, vg_stream_t stream);

/* The fp8 K/V cache of the decode step.  Format: OCP e4m3 (torch.float8_e4m3fn), one byte per element, NO scale; layout
 *   [max_len, Hkv, D] uint8 — the bf16 cache's layout with one-byte elements.  The value quantised is the bf16 value the bf16 cache would have held,
 *   clamped to +-448 in fp32 and rounded to nearest even: bit for bit x.float().clamp(-448, 448).to(torch.float8_e4m3fn); a NaN stays a NaN code.
 *   (Premise: K after RoPE and V are O(1) - O(100); magnitudes above 448 saturate, magnitudes of 2^-10 and below flush to zero.)
 * vg_kv_quantize_fp8: dst[i] = that code of src[i] (bf16), i < n; src / dst 4-byte aligned.  Used after a prefill on the rows it wrote.
 * vg_decode_attention_kv8: vg_decode_attention (same arguments, same workspace) with bf16 qkv / out and uint8 caches (8-byte aligned).  Every sum runs
 *   in the bf16 kernel's order on the exactly converted codes, so the result is bit-identical to vg_decode_attention on the dequantised caches.  The
 *   new token's key / value take part in their own step unquantised; the row appended at *pos_dev is their quantised form.  Shapes: dtype VG_BF16,
 *   H / Hkv in {1, 2, 4, 8}, D % 8 == 0, D <= 256 (vg_decode_attention_kv8_supported); keys_per_wg as vg_decode_attention. */
int vg_kv_quantize_fp8(const void* src, uint8_t* dst, int64_t n, vg_stream_t stream);
int vg_decode_attention_kv8_supported(int H, int Hkv, int D, int dtype);
int vg_decode_attention_kv8(const void* qkv, void* k_cache, void* v_cache, const float* cos, const float* sin, void* out, int H, int Hkv, int D,
                            int max_len, int window, float scale, const int* pos_dev, float* workspace, int64_t ws_floats, int keys_per_wg,
                            int dtype, vg_stream_t stream);

/* r06— the decode step with the RoPE in the projection and the attention as a wave-private flash pass (bf16, head_dim 128):
 * vg_decode_qkv_rope: q|k|v projection of the new token (RMSNorm fused as in vg_decode_gemv) with rotate-half RoPE of the q and k heads and the
 *   KV-cache append in the GEMV's epilogue: q_out [H*D] receives the rotated query heads, k_cache / v_cache ([max_len,Hkv,D]) row *pos_dev the
 *   rotated key / the value row.  rope_cs: fp32 [2][D/2] = cos row | sin row of position *pos_dev (kept current by vg_decode_advance).
 *   Replaces HF LlamaAttention.forward's q_proj / k_proj / v_proj + apply_rotary_pos_emb + cache update at q_len = 1
 *   (R/model/videogpt_plus/model/language_model/llama3_1.py:40-108 via generate).
 * vg_decode_attention2: softmax(q.K[lo..p]^T * scale).V[lo..p] for the pre-rotated q against caches that already hold row p; keys_per_wg 128 / 256.
 *   The caches must hold FINITE values in every row (allocate them zero-filled): rows past p are masked, not skipped.  workspace: the
 *   vg_decode_attention one (zero-filled once; the last Hkv words are self-resetting counters).
 * vg_decode_advance: the decode loop's bookkeeping on the device.  tok / step given (both or neither) — k = *step; raw[k] = *tok; *tok = forced[k] >= 0 ?
 *   forced[k] : *tok; hist[k] = *tok; *step = k + 1 — then *pos += inc (0 / 1); rope_cs given — rope_cs = rows *pos of cos / sin ([max_len, half_dim],
 *   after the increment).  forced / hist / raw may be NULL.  What HF generate()'s loop does on the host between two forward calls (logits
 *   processor, input_ids append, cache_position + 1). */
int vg_decode_qkv_rope_supported(int H, int Hkv, int D, int K, int dtype);
int vg_decode_qkv_rope(const void* x, const void* Wqkv, int64_t ldw, const float* norm_w, float eps, void* q_out, void* k_cache,
                       void* v_cache, const float* rope_cs, const int* pos_dev, int H, int Hkv, int D, int K, int dtype,
                       vg_stream_t stream);
int vg_decode_attention2_supported(int H, int Hkv, int D, int dtype);
int vg_decode_attention2(const void* q, const void* k_cache, const void* v_cache, void* out, int H, int Hkv, int D, int max_len,
                         int window, float scale, const int* pos_dev, float* workspace, int64_t ws_floats, int keys_per_wg, int dtype,
                         vg_stream_t stream);
/* The head and tail of a captured decode step in one launch each: vg_decode_step_begin — x = table[*tok] (vg_embed of one row) and rope_cs = rows *pos of cos /
 *   sin (rope_cs may be NULL); vg_argmax_partial — vg_argmax's first stage: packed (value, ~index) keys atomicMax-ed into acc[row], acc zero on entry;
 *   vg_decode_step_end — *tok = index decoded from acc[0] (acc[0] left zero), hid_all[*pos] = row (vg_store_row), then vg_decode_advance's bookkeeping with
 *   inc = 1.  Same results as vg_embed, vg_decode_advance, vg_argmax, vg_store_row, vg_decode_advance in that order. */
int vg_decode_step_begin(const int64_t* tok, const void* table, void* x, int D, int dtype, const int* pos, const float* cos, const float* sin,
                         float* rope_cs, int half_dim, vg_stream_t stream);
int vg_argmax_partial(const void* x, int64_t rows, int n, uint64_t* acc, int dtype, vg_stream_t stream);
int vg_decode_step_end(uint64_t* acc, int64_t* tok, int* pos, int* step, const int64_t* forced, int n_forced, int64_t* hist, int64_t* raw, int cap,
                       const void* row, void* hid_all, int D, int dtype, vg_stream_t stream);
int vg_decode_advance(int64_t* tok, int* pos, int* step, const int64_t* forced, int n_forced, int64_t* hist, int64_t* raw, int cap,
                      const float* cos, const float* sin, float* rope_cs, int half_dim, int inc, vg_stream_t stream);
/* The batched multi-prompt decode step: B <= 16 rows, each bit-identical to the single-row kernel on that row alone.
 * vg_decode_rows_supported: 1 when the B-row kernels below cover a bf16 Llama layer of this shape (head_dim 128; hidden / inter multiples of 2048).
 * vg_decode_gemv_rows: vg_decode_gemv for B rows x[b] = x + b * ldx -> y + b * ldy (residual R + b * ldr); bf16 only, K = 3072 or 2048 x {1, 2, 4, 7, 8}.
 * vg_decode_qkv_rope_rows: vg_decode_qkv_rope for B rows: row b at position pos[b] with rope_cs + b * D (cos row | sin row), q -> q_out + b * ldq,
 *   its key / value rows into slot b: k_slots / v_slots + b * slot_stride + (pos[b] - row0) * Hkv * D (rows clamped to [0, slot_rows)).
 * vg_decode_attention2_rows: vg_decode_attention2 for B rows (q / out rows of H * D); key rows below row0 (a multiple of keys_per_wg) from
 *   k_cache / v_cache ([max_len, Hkv, D], shared), rows from row0 on from slot b as above.  n_bound: every pos[b] < n_bound <= row0 + slot_rows over
 *   the launches (the grid's splits).  workspace: vg_decode_attention2_rows_ws_floats() floats, zero-filled once.
 * vg_decode_step_begin_rows / vg_decode_step_end_rows: vg_decode_step_begin / vg_decode_step_end per row b: tok / pos / step / acc [b], x / row + b * D,
 *   rope_cs + b * 2 * half_dim, forced / hist / raw + b * n_forced / cap, final-norm row of position p into hid + b * hid_stride + (p - hid_row0) * D
 *   (rows clamped to [0, hid_rows)). */
int vg_decode_rows_supported(int H, int Hkv, int D, int hidden, int inter, int dtype);
int vg_decode_gemv_rows(const void* x, int64_t ldx, const void* W, int64_t ldw, void* y, int64_t ldy, const float* norm_w, float eps,
                        const void* R, int64_t ldr, int N, int K, int B, int glu, int dtype, vg_stream_t stream);
/* The B-row projections of the decode mode decode_gemv = "mfma" (DESIGN.md section 11): y[b] = f(x[b]) . W^T (+ R[b]) on v_mfma_f32_16x16x32_bf16.
 * Arguments as vg_decode_gemv_rows; x bf16, W bf16 [N or 2N, K] read in place, y / R of out_dtype (VG_BF16 | VG_F32).  B in [1, 16]: the batch is
 * always one 16-row operand whose rows >= B are zeros, and neither the K walk nor the order of the partial sums depends on B, so row b of a B-row
 * call is bit-identical to the one-row call on row b, whatever the other rows hold (the single-row step of the mode calls this with B = 1).
 * Sums: fp32, k ascending inside each of four K slices, the slices added in order.  norm_w: RMSNorm prologue with vg_decode_gemv's roundings
 * (equal to vg_rmsnorm followed by the plain call), K <= 4096 only, VG_ERR_UNSUPPORTED beyond.  glu: SwiGLU epilogue of vg_decode_gemv.
 * K one of 3072, 4096, 8192, 14336, any N > 0 (per half when glu; a last tile of fewer than 16 weight rows re-reads row N - 1 and stores nothing
 * for the missing rows) (vg_decode_gemm_rows_supported(N, K) != 0), VG_ERR_UNSUPPORTED otherwise.  x, W and norm_w 16-byte aligned, ldx / ldw multiples of 8.  No workspace and no communication between workgroups. */
int vg_decode_gemm_rows_supported(int N, int K);
int vg_decode_gemm_rows(const void* x, int64_t ldx, const void* W, int64_t ldw, void* y, int64_t ldy, const float* norm_w, float eps,
                        const void* R, int64_t ldr, int N, int K, int B, int glu, int out_dtype, vg_stream_t stream);
/* vg_decode_gemm_rows on quantised weights (the decode mode decode_gemv = "mfma_q", DESIGN.md sections 8 and 11): the same walk on
 * v_mfma_f32_16x16x32_bf16, the weight bytes converted to bf16 operand registers on the way (v_cvt_scalef32_pk_bf16_fp8 / _fp4: exact), so the
 * VALU work per weight is half an instruction whatever B is.  The operands are those of vg_decode_gemv_w8_rows / vg_decode_gemv_w4_rows:
 *   W8 [N or 2N, K] OCP e4m3 with one fp32 scale per weight row: converted with scale 1.0, wscale[n] multiplies the fp32 total in the epilogue
 *     (before the gate / up rounding of the glu form), as vg_decode_gemv_w8; ldw a multiple of 16, >= K.
 *   W4: the PACKED MXFP4 rows of vg_decode_gemv_w4 read in place (row n at W4 + n * ldw_bytes = a head of 64 * SPL scale bytes, then K / 2 code
 *     bytes; ldw_bytes a multiple of 16 that covers the row).  The block scale 2^(s - 127) goes into the conversion; a lane's 16-byte load is one
 *     scale block.  A scale byte 0 means the block is EXACTLY zero, whatever its codes hold (the kernel converts +0 codes in their place: the
 *     conversion instruction reads only the exponent field of the float s << 23, so 0.0f alone would act as 2^-127).
 *     The heads of a workgroup's rows are read once, ahead of the walk, with 16-byte loads.
 * Everything else is vg_decode_gemm_rows' contract: x bf16, y / R of out_dtype (VG_BF16 | VG_F32); B in [1, 16], the batch always one 16-row
 * operand whose rows >= B are zeros; K one of 3072, 4096, 8192, 14336 and any N > 0 (per half when glu; a ragged last tile re-reads row N - 1 and
 * stores nothing for the missing rows) (vg_decode_gemm_w8_rows_supported / _w4_rows_supported(N, K) != 0), VG_ERR_UNSUPPORTED otherwise; the
 * norm form at K <= 4096 only (VG_ERR_UNSUPPORTED beyond), equal to vg_rmsnorm followed by the plain call; x, W and norm_w 16-byte aligned,
 * ldx a multiple of 8, VG_ERR_ARG otherwise.  No workspace, no communication between workgroups.
 * Row b of a B-row call is bit-identical to the one-row call on row b, whatever the other rows hold, +-Inf / NaN included.  Sums are fp32, k
 * ascending inside each of four K slices in the kernel's fixed k order (vg_decode_mfma.hip), the slices added in order ((s0 + s1) + s2) + s3;
 * nothing depends on B.  Roundings: the epilogue of vg_decode_gemv (gate / up / silu to bf16, residual in the output dtype, one output rounding).
 * NOT bit-identical to vg_decode_gemv_w8_rows / _w4_rows: the products are the same exact values, summed in another order. */
int vg_decode_gemm_w8_rows_supported(int N, int K);
int vg_decode_gemm_w8_rows(const void* x, int64_t ldx, const uint8_t* W8, int64_t ldw, const float* wscale, void* y, int64_t ldy,
                           const float* norm_w, float eps, const void* R, int64_t ldr, int N, int K, int B, int glu, int out_dtype,
                           vg_stream_t stream);
int vg_decode_gemm_w4_rows_supported(int N, int K);
int vg_decode_gemm_w4_rows(const void* x, int64_t ldx, const uint8_t* W4, int64_t ldw_bytes, void* y, int64_t ldy, const float* norm_w, float eps,
                           const void* R, int64_t ldr, int N, int K, int B, int glu, int out_dtype, vg_stream_t stream);
/* vg_decode_gemv_w8 for B rows (the MLP and the lm_head of the batched step with fp8 decode weights): x[b] = x + b * ldx (bf16, K elements),
 * W8 [N or 2N, K] fp8 e4m3 with one fp32 scale per weight row, y[b] = y + b * ldy (out_dtype VG_BF16 | VG_F32), residual R + b * ldr of the output
 * dtype, norm_w / eps and glu as vg_decode_gemv_w8.  Row b is bit-identical to vg_decode_gemv_w8 on row b alone; every weight chunk is read once.
 * B in [1, 16], staged in buckets of 1, 2, 4, 8, 16 rows; K must be one of 3072, 4096, 8192, 14336 (vg_decode_gemv_w8_rows_supported(K) != 0);
 * x, W8 and norm_w 16-byte aligned, ldx a multiple of 8, ldw of 16.  LDS: without a norm the rows are staged in phases of at most 64 KiB; with a
 * norm the whole rows of the bucket are staged, so bucket x K x 2 bytes must fit 152 KiB (K <= 4096 at 16 rows), VG_ERR_UNSUPPORTED otherwise. */
int vg_decode_gemv_w8_rows_supported(int K);
int vg_decode_gemv_w8_rows(const void* x, int64_t ldx, const uint8_t* W8, int64_t ldw, const float* wscale, void* y, int64_t ldy,
                           const float* norm_w, float eps, const void* R, int64_t ldr, int N, int K, int B, int glu, int out_dtype,
                           vg_stream_t stream);
int vg_decode_qkv_rope_rows(const void* x, int64_t ldx, const void* Wqkv, int64_t ldw, const float* norm_w, float eps, void* q_out, int64_t ldq,
                            void* k_slots, void* v_slots, int64_t slot_stride, int row0, int slot_rows, const float* rope_cs, const int* pos,
                            int H, int Hkv, int D, int K, int B, int dtype, vg_stream_t stream);
int64_t vg_decode_attention2_rows_ws_floats(int H, int Hkv, int D, int n_bound, int keys_per_wg, int B);
int vg_decode_attention2_rows(const void* q, const void* k_cache, const void* v_cache, int max_len, const void* k_slots, const void* v_slots,
                              int64_t slot_stride, int row0, int slot_rows, void* out, int H, int Hkv, int D, int n_bound, int window, float scale,
                              const int* pos, float* workspace, int64_t ws_floats, int keys_per_wg, int B, int dtype, vg_stream_t stream);
int vg_decode_step_begin_rows(const int64_t* tok, const void* table, void* x, int D, int dtype, const int* pos, const float* cos, const float* sin,
                              float* rope_cs, int half_dim, int B, vg_stream_t stream);
int vg_decode_step_end_rows(uint64_t* acc, int64_t* tok, int* pos, int* step, const int64_t* forced, int n_forced, int64_t* hist, int64_t* raw,
                            int cap, const void* row, void* hid, int64_t hid_stride, int hid_row0, int hid_rows, int D, int dtype, int B, vg_stream_t stream);
/* The batched step of the decode_attention path (Phi-3-mini width), each row bit-identical to the single-row kernel on it alone.
 * vg_decode_attention_rows_supported: 1 when vg_decode_attention_rows covers the shape (bf16, MHA, head_dim 96).
 * vg_decode_step_rows_supported: 1 when the B-row kernels cover a whole layer of the decode_attention step: the attention above, hidden = H * D
 *   (q|k|v, o, gate|up GEMVs) and inter (down) row lengths of vg_decode_gemv_rows.
 * vg_decode_attention_rows: vg_decode_attention for B rows: row b's q|k|v row at qkv + b * ldqkv, RoPE at pos[b] (cos / sin: [>= max_len, D / 2]),
 *   its new key / value row appended into slot b: k_slots / v_slots + b * slot_stride + (pos[b] - row0) * Hkv * D; key rows below row0 (a multiple
 *   of 128) from k_cache / v_cache ([max_len, Hkv, D], shared), rows from row0 on from slot b; output row b at out + b * H * D.  Keys per workgroup
 *   of row b: 128 when pos[b] >= kpw_min, else 64.  n_bound: every pos[b] < n_bound <= min(row0 + slot_rows, max_len) (a row outside
 *   [row0, n_bound) is skipped).  workspace: vg_decode_attention_rows_ws_floats() floats, zero-filled once (self-resetting counters). */
int vg_decode_attention_rows_supported(int H, int Hkv, int D, int dtype);
int vg_decode_step_rows_supported(int H, int Hkv, int D, int hidden, int inter, int dtype);
int64_t vg_decode_attention_rows_ws_floats(int H, int Hkv, int D, int n_bound, int B);
int vg_decode_attention_rows(const void* qkv, int64_t ldqkv, const void* k_cache, const void* v_cache, int max_len, void* k_slots, void* v_slots,
                             int64_t slot_stride, int row0, int slot_rows, const float* cos, const float* sin, void* out, int H, int Hkv, int D,
                             int n_bound, int window, float scale, const int* pos, int kpw_min, float* workspace, int64_t ws_floats, int B, int dtype,
                             vg_stream_t stream);
/* vg_decode_attention_rows_kv8: vg_decode_attention_rows on the fp8 K/V format above — the shared caches AND the slots hold e4m3 codes (uint8);
 *   slot_stride is in elements, which are bytes.  Same arguments, workspace and shapes (bf16 qkv / out, MHA, head_dim 96); row b is bit-identical to
 *   vg_decode_attention_kv8 on that row alone with the whole cache in one array. */
int vg_decode_attention_rows_kv8_supported(int H, int Hkv, int D, int dtype);
int vg_decode_attention_rows_kv8(const void* qkv, int64_t ldqkv, const void* k_cache, const void* v_cache, int max_len, void* k_slots, void* v_slots,
                                 int64_t slot_stride, int row0, int slot_rows, const float* cos, const float* sin, void* out, int H, int Hkv, int D,
                                 int n_bound, int window, float scale, const int* pos, int kpw_min, float* workspace, int64_t ws_floats, int B,
                                 int dtype, vg_stream_t stream);
/* The fp8 K/V format above on the rope step (cfg kv_cache = "fp8_rope"): bf16 activations, uint8 e4m3 caches and slots in
 *   the [rows, Hkv, D] layout, 8-byte aligned; slot_stride in elements (= bytes), a multiple of 8.  Everything not named here is the bf16 entry
 *   point's: arguments, shapes, workspaces (vg_decode_attention_ws_floats / vg_decode_attention2_rows_ws_floats), premises.
 * vg_decode_qkv_rope_kv8 / _rows_kv8: vg_decode_qkv_rope / _rows with byte K/V destinations.  q_out is bit-identical; the key / value row written
 *   at *pos_dev (slot row pos[b] - row0, clamped) holds the codes of the bf16 row the bf16 entry point writes (quantised after its bf16 rounding:
 *   clamp, nearest even, NaN kept); no other byte of the caches is touched.  bf16 only, K in {2048, 4096}; fp32 is VG_ERR_UNSUPPORTED.
 * vg_decode_attention2_kv8 / _rows_kv8: vg_decode_attention2 / _rows on such caches.  The codes are converted exactly (K to packed bf16, V to fp32)
 *   and every sum runs in the bf16 kernel's order, so the output is bit-identical to the bf16 entry point on the dequantised caches and slots.
 *   Every row finite (a zero byte is +0.0: zero-filled caches satisfy it); rows past the position are masked, not skipped.
 *   vg_decode_attention2_kv8_supported = vg_decode_attention2_supported (bf16, D = 128, H / Hkv in {1, 2, 4, 8}); keys_per_wg 128 / 256.
 * Unlike vg_decode_attention_kv8, where the new token's key / value take part in their own step unquantised, here they are in the cache before the
 *   attention launch reads it: the new token attends to its own key / value already quantised. */
int vg_decode_qkv_rope_kv8(const void* x, const void* Wqkv, int64_t ldw, const float* norm_w, float eps, void* q_out, uint8_t* k_cache,
                           uint8_t* v_cache, const float* rope_cs, const int* pos_dev, int H, int Hkv, int D, int K, int dtype,
                           vg_stream_t stream);
int vg_decode_qkv_rope_rows_kv8(const void* x, int64_t ldx, const void* Wqkv, int64_t ldw, const float* norm_w, float eps, void* q_out, int64_t ldq,
                                uint8_t* k_slots, uint8_t* v_slots, int64_t slot_stride, int row0, int slot_rows, const float* rope_cs,
                                const int* pos, int H, int Hkv, int D, int K, int B, int dtype, vg_stream_t stream);
int vg_decode_attention2_kv8_supported(int H, int Hkv, int D, int dtype);
int vg_decode_attention2_kv8(const void* q, const uint8_t* k_cache, const uint8_t* v_cache, void* out, int H, int Hkv, int D, int max_len,
                             int window, float scale, const int* pos_dev, float* workspace, int64_t ws_floats, int keys_per_wg, int dtype,
                             vg_stream_t stream);
int vg_decode_attention2_rows_kv8(const void* q, const uint8_t* k_cache, const uint8_t* v_cache, int max_len, const uint8_t* k_slots,
                                  const uint8_t* v_slots, int64_t slot_stride, int row0, int slot_rows, void* out, int H, int Hkv, int D, int n_bound,
                                  int window, float scale, const int* pos, float* workspace, int64_t ws_floats, int keys_per_wg, int B, int dtype,
                                  vg_stream_t stream);
/* Sampled decoding (csrc/vg_sample.hip): HF's Temperature -> TopK -> TopP warpers and the draw on one fp32 logits row x[n]
 *   (n < 2^22), one launch.  params: the 24-byte device block {float T; float p; int k; int pad; uint64 seed} (k = 0: no top-k; p = 1: no top-p).
 * vg_sample_partial — acc[0] = the drawn entry's packed (ordered value bits, ~index) key, the hand-off vg_argmax_partial leaves, so
 *   vg_decode_step_end consumes it.  fast_ws == NULL: the general route (one 1024-thread workgroup, any k).  fast_ws != NULL: the fast route
 *   for 1 <= k <= 64 and n <= 131072 (up to 64 workgroups + a last-arriver merge; tie overflow or another k falls back to the general route
 *   inside the launch); fast_ws = vg_sample_workspace_ints() int32, zero-filled once, one per stream (its ticket resets itself).  tok != NULL: *tok = the drawn index as well (either may be NULL, not both).  u = (philox4x32_10(key = seed, counter = (*step, 0, 0, 0))[0] >> 8) * 2^-24, or *u_override when not NULL (tests).
 * vg_sample_partial_rows — vg_sample_partial on the B rows x[b * ldx .. b * ldx + n) of a batched decode step in ONE launch (ldx in elements, >= n).
 *   Row b reads params + 24 b bytes, step[b] and (when not NULL) u_override[b], and writes acc[b] and / or tok[b]; each is bit-identical to
 *   vg_sample_partial on row b alone.  fast_ws == NULL: one 1024-thread workgroup per row.  fast_ws != NULL: up to 64 workgroups per row;
 *   fast_ws = B * vg_sample_workspace_ints() int32, zero-filled once — row b's candidates and self-resetting ticket live in its own slice, and a
 *   tie overflow or a k outside 1..64 sends that row alone to the general route inside the launch.  1 <= B <= 65535.
 * vg_sample_survivors — the entries the warpers keep: idx[j] / prob[j] for j < min(*count, cap), in no particular order; *count (zero on entry)
 *   receives their number.  prob = softmax over the kept entries.
 * vg_sample_philox — out[i] = philox4x32_10(key = seeds[i], counter = (steps[i], 0, 0, 0))[0]. */
int vg_sample_workspace_ints(void);
int vg_sample_partial(const float* x, int n, const void* params, const int* step, const float* u_override, uint64_t* acc, int64_t* tok,
                      int* fast_ws, vg_stream_t stream);
int vg_sample_partial_rows(const float* x, int64_t ldx, int n, int B, const void* params, const int* step, const float* u_override, uint64_t* acc,
                           int64_t* tok, int* fast_ws, vg_stream_t stream);
int vg_sample_survivors(const float* x, int n, const void* params, int64_t* idx, float* prob, int cap, int* count, vg_stream_t stream);
int vg_sample_philox(const uint64_t* seeds, const int* steps, int n, uint32_t* out, vg_stream_t stream);
/* Per-token scores (csrc/vg_scores.hip): for the B rows x[b * ldx .. b * ldx + n) of fp32 logits (1 <= B <= 16, n >= 2,
 *   ldx >= n in elements, finite inputs), ONE launch that reads no host value and can be captured into a graph.  Per row:
 *   top1, top2 — the indices of the largest and the second-largest entry; ties go to the lower index, with a tied maximum top2 is the
 *     second-lowest index that holds it (-0 counts as +0);
 *   margin = x[top1] - x[top2], one fp32 subtraction: >= 0, exactly 0 on a tie;
 *   logprob = log_softmax(x)[pick] on the raw logits (no temperature, no warpers).  The pick is the index in the packed key acc[b] that
 *     vg_argmax_partial / vg_sample_partial* leave (read, not cleared), or tok[b]: exactly one of acc / tok is not NULL.  A pick outside
 *     [0, n) gives logprob = NaN.
 *   Slot j = step[b] (device int32: the counter the sampler reads, the index of the token being emitted; 0 = the prefill's token) receives
 *   scores[b, j, 0..1] = (logprob, margin) (float32) and top2[b, j, 0..1] = (top1, top2) (int64); both arrays are [B, cap, 2].  j outside
 *   [0, cap) writes nothing; no other element of either array is touched.
 *   Determinism: row b of a B-row launch equals the one-row launch on that row bit for bit, and two launches on one input are bit-equal.  Up to
 *   64 workgroups per row (slices of <= 2048 entries); a slice's softmax mass is vg_sample's fixed point, sum floor(expf(x - m) * 2^40) in
 *   uint64 with m the slice's maximum (independent of the order of its terms); the row's last workgroup to arrive (self-resetting ticket)
 *   rescales the slices' masses to the row's maximum in float64 and adds them in slice order.  The slicing is a function of n alone.
 *   ws: B * vg_token_scores_workspace_ints() int32, zero-filled once, row b works in its own slice; may be NULL for n <= 2048 (one workgroup
 *   per row).  VG_ERR_ARG without a launch: NULL x / scores / top2 / step, both or neither of acc / tok, n < 2, B outside 1..16, ldx < n,
 *   cap <= 0, NULL ws with n > 2048. */
int vg_token_scores_workspace_ints(void);
int vg_token_scores_rows(const float* x, int64_t ldx, int n, int B, const uint64_t* acc, const int64_t* tok, const int* step, float* scores,
                         int64_t* top2, int cap, int* ws, vg_stream_t stream);

/* vg_decode_layer (r03): everything of a decoder layer behind the q|k|v projection as ONE launch — vg_decode_attention, then
 *   y_o = attn_out . Wo^T + resid (vg_decode_gemv), and when Wgu != NULL also act = SwiGLU(RMSNorm(y_o; norm_w, eps) . Wgu^T) and
 *   y = act . Wdown^T + y_o.  The GEMV workgroups request their weight rows before the row they multiply exists and wait for it on
 *   device-side arrival counters (csrc/vg_decode.hip: decode_layer_kernel), so the weight stream no longer idles behind the
 *   latency-bound attention and between the GEMVs.  Results are bit-identical to the separate calls.  The same zero-filled
 *   workspace as vg_decode_attention; flags: vg_decode_layer_flag_ints() ints, 128-byte aligned, zero-filled by the caller before
 *   EVERY launch (one memset per token over the regions of all layers); word [1] != 0 afterwards = a device-side wait gave up.
 *   vg_decode_layer_roles: 0 = shape not covered (use the separate calls), 1 = attention + o_proj
 *   (pass Wgu = NULL), 3 = the MLP as well.  HF LlamaDecoderLayer.forward at q_len = 1 (R/model/VideoGLaMM.py:616-628 via generate). */
int vg_decode_layer_roles(int H, int Hkv, int D, int hidden, int inter, int dtype);
int64_t vg_decode_layer_flag_ints(void);
int vg_decode_layer(const void* qkv, void* k_cache, void* v_cache, const float* cos, const float* sin, void* attn_out,
                    int H, int Hkv, int D, int max_len, int window, float scale, const int* pos_dev,
                    float* workspace, int64_t ws_floats, int32_t* flags,
                    const void* Wo, int64_t ldo, const void* resid, void* y_o,
                    const float* norm_w, float eps, const void* Wgu, int64_t ldgu, void* act,
                    const void* Wdown, int64_t lddown, void* y, int hidden, int inter, int dtype, vg_stream_t stream);

/* ---- row normalisation -------------------------------------------------------------------------
 * LayerNorm over the last dim (biased variance, two-pass fp32): nn.LayerNorm and LayerNorm2d
 * (R/model/segment_anything_2/sam2/modeling/sam2_utils.py:137-149 — channels-last makes them identical).
 * RMSNorm: R/model/videogpt_plus/model/internvideo/internvideo2.py:134-145 and HF LlamaRMSNorm.
 * x rows have stride ldx elements, y rows ldy.
 */
int vg_layernorm(const void* x, int64_t ldx, const float* w, const float* b, void* y, int64_t ldy,
                 int64_t rows, int C, float eps, int in_dtype, int out_dtype, vg_stream_t stream);
int vg_rmsnorm(const void* x, int64_t ldx, const float* w, void* y, int64_t ldy, int64_t rows, int C,
               float eps, int in_dtype, int out_dtype, vg_stream_t stream);

/* ---- SAM2 two-way transformer, image side of the image -> token cross-attention, fused (r04) --------
 * Replaces, for the 4096 image rows of every (frame, object) instance, the chain q_proj -> Attention (8 heads x 16, keys = the nt prompt/output
 * tokens) -> out_proj -> + residual -> LayerNorm -> + dense PE of TwoWayAttentionBlock.forward
 * (R/model/segment_anything_2/sam2/modeling/sam/transformer.py:185-193 with Attention.forward :236-260) by one pass over the rows:
 *   s = xpe . u2^T + c2  (columns (head h, token t) = h * TP + t),  a = softmax over t < nt inside each head,  y = a . w2t^T + bo,
 *   x_out = LayerNorm(x + y),  xpe_out = x_out + pe.
 * u2 [N, 8 TP, 256], c2 [N, 8 TP] (fp32), w2t [N, 256, 8 TP] carry the token side (k / v projections folded into the q / out projection weights:
 * videoglamm_amd/sam2.py:_i2t_fused); x_out, xpe_out [N, P, 256]; xpe, x [x_instances, P, 256] — instance n reads slot n % x_instances (the first
 * block of a frame's objects shares the frame's embedding); pe [P, 256]; bf16 only; TP = 8 or 16; nt <= TP.
 */
int vg_twoway_image_update(const void* xpe, const void* x, const void* u2, const float* c2, const void* w2t, const float* bo,
                           const float* ln_w, const float* ln_b, float eps, const void* pe, void* x_out, void* xpe_out,
                           int N, int x_instances, int P, int nt, int TP, int dtype, vg_stream_t stream);
/* Token-side layout of the fused two-way path: gather = 0: x [N, nt, 128] -> out [N, 8, TP, 128], row (h, t) = head h's 16 channels of token t,
 * zeros elsewhere (the per-head products of Attention.forward, sam/transformer.py:236-260, as ONE small GEMM on block-diagonal rows);
 * gather = 1: the inverse read — x [N, 8, TP, 128] -> out [N, nt, 128], channel c of token t from row (c / 16, t).  bf16 / fp32. */
int vg_heads_blockdiag(const void* x, void* out, int N, int nt, int TP, int gather, int dtype, vg_stream_t stream);

/* Output upscaling + hypernetwork product of the mask decoder, fused (r04): MaskDecoder.predict_masks
 * (R/model/segment_anything_2/sam2/modeling/sam/mask_decoder.py:225-245): ConvTranspose2d(256 -> 64, k2 s2) + feat_s1 -> LayerNorm2d -> GELU ->
 * ConvTranspose2d(64 -> 32, k2 s2) + feat_s0 -> GELU -> masks[k] = hyper_in[k] . upscaled (k = 0..3).
 * x [N, es*es, 256] (the two-way transformer's image output); w0 [4*64, 256], w1 [4*32, 64]: the ConvT weights as GEMM weights, row (dy*2+dx)*Cout + co
 * (Params.convT_w); s1 [images, (2es)^2, 64], s0 [images, (4es)^2, 32] channels-last, instance n uses image n % images; hyper [N, 4, 32];
 * masks fp32 [N, 4, 4es, 4es].  bf16 only.
 */
int vg_mask_upscale(const void* x, const void* w0, const float* b0, const void* s1, const float* ln_w, const float* ln_b, float eps,
                    const void* w1, const float* b1, const void* s0, const void* hyper, float* masks, int N, int images, int es, int dtype,
                    vg_stream_t stream);

/* ---- pointwise --------------------------------------------------------------------------------- */
/* out[i] = alpha*a[i] + beta*b[i % b_period]  (b may be NULL -> alpha*a[i] + beta) */
int vg_axpby(const void* a, const void* b, void* out, int64_t n, float alpha, float beta,
             int64_t b_period, int a_dtype, int b_dtype, int out_dtype, vg_stream_t stream);
/* y = act(x) */
int vg_activation(const void* x, void* y, int64_t n, int act, int in_dtype, int out_dtype,
                  vg_stream_t stream);
/* y[m,f] = silu(gu[m,f]) * gu[m,F+f]  (HF LlamaMLP: down(act(gate(x))*up(x)); gate|up packed) */
int vg_swiglu(const void* gu, void* y, int64_t M, int F, int dtype, vg_stream_t stream);
/* out = in converted */
int vg_cast(const void* in, void* out, int64_t n, int in_dtype, int out_dtype, vg_stream_t stream);
/* out[n,i] = cond[n] > 0 ? a[n,i] : (b ? b[i % b_period] : fill)   (fp32 cond); ld_out: elements between consecutive rows of out (0 = inner:
 * contiguous) — the object pointers go straight into their rows of the memory bank.
 * R/model/segment_anything_2/sam2/modeling/sam2_base.py:355-364,390-401 */
int vg_where_rows(const float* cond, const void* a, const void* b, void* out, int64_t rows,
                  int64_t inner, int64_t b_period, float fill, int64_t ld_out, int dtype, vg_stream_t stream);
/* mask fed to the memory encoder: out = (binarize ? (x>0) : sigmoid(x)) * scale + bias
 * R/model/segment_anything_2/sam2/modeling/sam2_base.py:684-693 */
int vg_mask_for_mem(const float* x, void* out, int64_t n, int binarize, float scale, float bias,
                    int out_dtype, vg_stream_t stream);
/* out[i] = x[i] > 0  (uint8)  R/model/VideoGLaMM.py:763,873 */
int vg_threshold(const float* x, uint8_t* out, int64_t n, vg_stream_t stream);
/* HF rotate-half RoPE, in place on x:[S,H,D] (token stride x_ss, head stride x_sh); cos/sin:[*,D/2] f32,
 * row used for token s is pos0+s.  HF modeling_llama.apply_rotary_pos_emb. */
int vg_rope_half(void* x, int64_t x_ss, int64_t x_sh, const float* cos, const float* sin, int S, int H,
                 int D, int pos0, int dtype, vg_stream_t stream);
/* SAM2 axial (complex-pair) RoPE, in place on x:[B,N,C] contiguous, only tokens n < n_rope;
 * token n uses table row n % n_grid.  cos/sin:[n_grid,C/2] f32.
 * R/model/segment_anything_2/sam2/modeling/position_encoding.py:174-216, sam/transformer.py:306-312 */
int vg_rope_axial(void* x, const float* cos, const float* sin, int B, int N, int C, int n_rope,
                  int n_grid, int dtype, vg_stream_t stream);
/* The same rotation on a STRIDED view holding H heads of Ch channels per row (bf16): x[b, n, h*Ch + c] at x + b*sb + n*ld (elements), every head
 * with the one [n_grid, Ch/2] table — the q | k columns of a fused q|k|v projection in one in-place launch (SAM2 memory self-attention, r04). */
int vg_rope_axial_heads(void* x, int64_t ld, int64_t sb, const float* cos, const float* sin, int B, int H, int Ch, int n_rope,
                        int n_grid, int dtype, vg_stream_t stream);
/* out[i,:] = table[ids[i],:]   (nn.Embedding) */
int vg_embed(const int64_t* ids, const void* table, void* out, int64_t n, int D, int dtype,
             vg_stream_t stream);
/* out[r] = first index of the row maximum (torch.argmax) (-0 counts as +0)  x:[rows,n] */
int vg_argmax(const void* x, int64_t rows, int n, int64_t* out, int dtype, vg_stream_t stream);

/* SAM2 mask selection, one call per decoder batch: masks fp32 [N,4,HW], ious fp32 [N,4], tokens [N,4,C].
 * mode 0: dynamic multimask via stability (R/.../sam/mask_decoder.py:247-295), token 0 returned;
 * mode 1: best predicted IoU among tokens 1..3 (R/.../sam2_base.py:376-386), that token returned.
 * out_mask [N,HW] fp32, out_iou [N] fp32, out_token [N,C] (may be NULL), out_idx [N] int32 (may be NULL). */
int vg_multimask_select(const float* masks, const float* ious, const void* tokens, float* out_mask,
                        float* out_iou, void* out_token, int* out_idx, int N, int64_t HW, int C, float delta,
                        float thresh, int mode, int token_dtype, vg_stream_t stream);

/* ---- spatial / layout (all NHWC) ---------------------------------------------------------------- */
/* 5-D gather copy: out (contiguous, dims n0..n4) = in at element strides s0..s4 */
int vg_permute5(const void* in, void* out, const int64_t dims[5], const int64_t strides[5], int dtype,
                vg_stream_t stream);
/* x:[B,H,W,C] -> cols:[B*Ho*Wo, Kpad], column (ky*kw+kx)*C + c, zero padded to Kpad.
 * Feeds vg_gemm for nn.Conv2d: hieradet patch embed (R/.../backbones/utils.py:65-95), MaskDownSampler
 * (R/.../memory_encoder.py:17-58), IV2/CLIP patch embeds. */
int vg_im2col(const void* x, void* cols, int B, int H, int W, int C, int kh, int kw, int stride,
              int pad, int Kpad, int dtype, vg_stream_t stream);
/* depthwise kxk conv, stride 1, pad k/2, NHWC; w:[k*k, C] f32, bias:[C] f32  (CXBlock dwconv,
 * R/.../memory_encoder.py:81-87) */
int vg_dwconv(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int C,
              int k, int dtype, vg_stream_t stream);
/* Conv2d(k = 3, stride 2, pad 1) + bias -> LayerNorm over the channels (eps) -> GELU(erf) in ONE pass, channels-last:
 * x:[B,H,W,Cin] -> y:[B,(H+1)/2,(W+1)/2,Cout]; w:[Cout, ldw] in the tensors' dtype with column (ky*3+kx)*Cin + c (vg_im2col's column order);
 * bias / ln_w / ln_b fp32.  The few-channel stages of SAM2's MaskDownSampler (R/.../memory_encoder.py:17-63: 1->4->16 channels at
 * 512^2 / 256^2 outputs, LayerNorm2d + GELU after every conv) — built for exactly the pairs 1->4 and 4->16, VG_ERR_UNSUPPORTED otherwise. */
int vg_conv3s2_ln_gelu(const void* x, const void* w, int64_t ldw, const float* bias, const float* ln_w, const float* ln_b, float eps,
                       void* y, int B, int H, int W, int Cin, int Cout, int dtype, vg_stream_t stream);
/* ConvTranspose2d k2 s2 tail: g:[B,H,W,4,C] (GEMM output, tap = dy*2+dx) -> y:[B,2H,2W,C] (+bias)
 * R/.../sam/mask_decoder.py:64-73 */
int vg_pixel_shuffle2(const void* g, const float* bias, void* y, int B, int H, int W, int C, int dtype,
                      vg_stream_t stream);
/* 2x2 stride-2 max / mean pooling over an NHWC grid (Hiera q-pool hieradet.py:20-34,64-66;
 * adaptive_avg_pool2d with integer ratio 2, R/model/videogpt_plus/model/arch.py:88-96) */
int vg_pool2(const void* x, void* y, int B, int H, int W, int C, int64_t x_pix_stride, int is_max,
             int dtype, vg_stream_t stream);
/* window partition with zero padding / reverse with crop (R/.../backbones/utils.py:16-62) */
int vg_window_partition(const void* x, void* win, int B, int H, int W, int C, int ws, int dtype,
                        vg_stream_t stream);
int vg_window_unpartition(const void* win, void* x, int B, int H, int W, int C, int ws, int dtype,
                          vg_stream_t stream);
/* bilinear resize, align_corners=False, no antialias, planar fp32 [N,Hi,Wi] -> [N,Ho,Wo]
 * (F.interpolate at sam2_base.py:368-374, sam2_video_predictor.py:509-516, VideoGLaMM.py:147-153) */
int vg_bilinear(const float* in, float* out, int N, int Hi, int Wi, int Ho, int Wo, vg_stream_t stream);
/* vg_bilinear + (logit > 0) in one pass: uint8 masks [N,Ho,Wo] (0 / 1) from low-resolution fp32 logits [N,Hi,Wi] — the final
 * `postprocess_masks(...) > 0` / `video_res_masks > 0.0` of R/model/VideoGLaMM.py:147-153,757-766,869-875 without materialising
 * the fp32 logits at output resolution.  Bit-identical to vg_threshold(vg_bilinear(x)). */
int vg_bilinear_mask(const float* in, uint8_t* out, int N, int Hi, int Wi, int Ho, int Wo, vg_stream_t stream);
/* y:[B,2H,2W,C] = lateral + nearest2x(top:[B,H,W,C])   (FPN top-down, image_encoder.py:113-127) */
int vg_upsample2_add(const void* lateral, const void* top, void* y, int B, int H, int W, int C,
                     int dtype, vg_stream_t stream);

/* vg_decode_gemv with fp8 weights (config C4's LLM path, decode side): W8:[N or 2N, K] bytes in OCP e4m3, one fp32
 * scale per weight row (w ~ scale[n] * fp8); x, the norm and the epilogue are unchanged (bf16 activations, fp32
 * accumulation): y[n] = scale[n] * sum_k fp8(W8[n,k]) * xn[k].  Halves the bytes a decode step streams.
 * K in {3072, 4096, 8192, 14336}. */
int vg_decode_gemv_w8(const void* x, const uint8_t* W8, int64_t ldw, const float* wscale, void* y, const float* norm_w,
                      float eps, const void* R, int N, int K, int glu, int out_dtype, vg_stream_t stream);
/* Lossless 13-bit form of bf16 weight rows for the decode GEMV.  Per weight: the byte [sign | c5 | m2] (an OCP e5m2 byte: c = E -
 * base_row in 1..30 for the biased bf16 exponent E, c = 0 = +-0; m2 = the two high mantissa bits) and the five low mantissa bits; per row the
 * fp32 scale 2^(base_row - 112).  A row is RAW — not represented; readers take it from the bf16 matrix — when its non-zero exponents span more
 * than 30 binades, when it holds a denormal, an inf or a NaN, or when its scale is no normal fp32.
 * Layout: row n = K / 2048 blocks of 3328 bytes at packed + n * vg_decode_pack13_row_bytes(K); block b covers K elements [2048 b, 2048 b + 2048)
 * as four lane-major planes, 64 x 16 B | 64 x 16 B | 64 x 16 B | 64 x 4 B = dwords H[0..3] | H[4..7] | L[0..3] | L[4] of lane 0..63.  The lane's
 * 32 weights are i = 8 u + j = element 8 (256 b + 64 u + lane) + j of the row (u < 4, j < 8): high byte in byte i % 4 of H[i / 4], low bits at
 * bits 5 i .. 5 i + 4 of the 160-bit little-endian string L.
 * vg_decode_pack13: W bf16 [N, K] (ldw elements, a multiple of 8; 16-byte aligned), K a multiple of 2048 -> packed, scale[N] (1 for a raw row) and
 * rawflag[N] (1 = raw; a raw row's block holds no meaning).  vg_decode_pack13_row_bytes: 0 for an unsupported K. */
int64_t vg_decode_pack13_row_bytes(int K);
int vg_decode_pack13(const void* W, int64_t ldw, int N, int K, uint8_t* packed, float* scale, uint8_t* rawflag, vg_stream_t stream);
/* the inverse: out bf16 [N, K] (ldo elements) from packed + scale, rows listed in raw[nraw] (int32) copied from W */
int vg_decode_unpack13(const uint8_t* packed, const float* scale, const int* raw, int nraw, const void* W, int64_t ldw, void* out, int64_t ldo,
                       int N, int K, vg_stream_t stream);
/* vg_decode_gemv (bf16 x, bf16 W) streaming the packed form of W instead of W: 13/16 of the bytes, the same bits.  The rows listed in raw[nraw]
 * are recomputed from W (which must stay the matrix that was packed).  K in {4096, 14336} (vg_decode_gemv_p13_supported), VG_ERR_UNSUPPORTED
 * otherwise; out_dtype VG_BF16 | VG_F32; x, the norm, glu, R and the epilogue as vg_decode_gemv. */
int vg_decode_gemv_p13_supported(int K);
int vg_decode_gemv_p13(const void* x, const void* W, int64_t ldw, const uint8_t* packed, const float* scale, const int* raw, int nraw, void* y,
                       const float* norm_w, float eps, const void* R, int N, int K, int glu, int out_dtype, vg_stream_t stream);
/* vg_decode_gemv with MXFP4 weights (OCP Microscaling v1.0; cfg decode_weights = "mxfp4", the MLP of the decode step — weight-only
 * quantisation of what R/chat.py:247-272 asks of bitsandbytes' load_in_4bit, in gfx950's own 4-bit format): blocks of 32 consecutive K elements of
 * a weight row share the scale 2^(s - 127) (one e8m0 byte s), the elements are e2m1 codes (bit 3 sign; magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6), element
 * 2j in the low nibble of byte j.  y[n] = sum_k 2^(s[n, k / 32] - 127) * e2m1(W4[n, k]) * xn[k]: each code is converted to bf16 with its scale
 * applied (exact), multiplied with the bf16 activation and summed in fp32; x, the norm, glu, R and the epilogue as vg_decode_gemv_w8.
 * K in {3072, 4096, 8192, 14336}, VG_ERR_UNSUPPORTED otherwise.  A block with s = 0 counts as zero.  Two layouts:
 *   scales != NULL: W4 row n = K / 2 code bytes at W4 + n * ldw_bytes; scales [rows, K / 32] contiguous, block b of row n at scales[n * K / 32 + b].
 *   scales == NULL (packed rows, the decoder's form): row n at W4 + n * ldw_bytes = a head of 64 * SPL scale bytes, then the K / 2 code bytes;
 *     SPL = 2 (K = 3072, 4096), 4 (8192), 8 (14336); head byte lane * SPL + u = the scale of block 64 u + lane (0 where K / 32 <= 64 u + lane):
 *     the scales one lane needs are one 2 / 4 / 8-byte load.
 * ldw_bytes a multiple of 16 that covers the row; x, W4, norm_w 16-byte aligned. */
int vg_decode_gemv_w4(const void* x, const uint8_t* W4, int64_t ldw_bytes, const uint8_t* scales, void* y, const float* norm_w, float eps,
                      const void* R, int N, int K, int glu, int out_dtype, vg_stream_t stream);
/* vg_decode_gemv_w4 for B rows (the MLP of the batched step with MXFP4 decode weights): x[b] = x + b * ldx (bf16, K elements), W4 PACKED rows only
 * (the decoder's form: row n at W4 + n * ldw_bytes = the head of 64 * SPL scale bytes, then the K / 2 code bytes; the separate-scales layout of the
 * single-row entry point is not needed here and has no B-row form), y[b] = y + b * ldy (out_dtype VG_BF16 | VG_F32), residual R + b * ldr of the
 * output dtype, norm_w / eps and glu as vg_decode_gemv_w4.  Row b is bit-identical to vg_decode_gemv_w4 on row b alone; every weight byte is read
 * once per launch and converted once for the B rows.  B in [1, 16], staged in buckets of 1, 2, 4, 8, 16 rows (a bucket row beyond B re-reads row
 * B - 1 and is not written); K must be one of 3072, 4096, 8192, 14336 (vg_decode_gemv_w4_rows_supported(K) != 0), VG_ERR_UNSUPPORTED otherwise;
 * ldw_bytes a multiple of 16 that covers a packed row, ldx a multiple of 8, x, W4 and norm_w 16-byte aligned.  LDS: without a norm the rows are
 * staged in phases of at most 64 KiB; with a norm the whole rows of the bucket are staged, so bucket x K x 2 bytes must fit 152 KiB (K <= 4096 at
 * 16 rows), VG_ERR_UNSUPPORTED otherwise. */
int vg_decode_gemv_w4_rows_supported(int K);
int vg_decode_gemv_w4_rows(const void* x, int64_t ldx, const uint8_t* W4, int64_t ldw_bytes, void* y, int64_t ldy, const float* norm_w, float eps,
                           const void* R, int64_t ldr, int N, int K, int B, int glu, int out_dtype, vg_stream_t stream);
/* vg_gemm for grids that leave most of the chip idle (few 128x128 tiles, long K): K is cut into ksplit slices that run as
 * separate workgroups, the fp32 partial tiles go to `workspace` (>= ksplit*M*N floats) and one pass sums them and applies
 * bias / act / gamma / residual.  Same result up to fp32 summation order.  M > 16, N % 8 == 0, no batch / GLU / window. */
int vg_gemm_splitk(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, const float* bias,
                   const float* gamma, const void* R, int64_t ldr, int M, int N, int K, int in_dtype, int out_dtype, int act,
                   int ksplit, float* workspace, int64_t ws_floats, vg_stream_t stream);
/* fp8 (OCP e4m3) prefill path of BASELINE config C4.
 * vg_quantize_fp8_rows: q[m,:] = e4m3(x[m,:] / scale[m]) with scale[m] = absmax(x[m,:]) / 448 (round to nearest even, what
 * torch's .to(float8_e4m3fn) does); x bf16 / fp32 [M,K], K % 4 == 0.
 * vg_gemm_f8: C[m,n] = scale_a[m] * scale_w[n] * sum_k A8[m,k] * W8[n,k]  (+ bias[n]) (+ R[m,n]), fp32 accumulation on
 * v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales (twice the bf16 MFMA rate at half the operand bytes);
 * a_op = 1: W8 = [gate; up] rows, C[m,n] = silu(gate)*up like vg_gemm.  M > 16 (prefill only), K % 16 == 0. */
int vg_quantize_fp8_rows(const void* x, int64_t ldx, uint8_t* q, int64_t ldq, float* scale, int64_t M, int K, int dtype,
                         vg_stream_t stream);
int vg_gemm_f8(const uint8_t* A8, int64_t lda, const float* a_scale, const uint8_t* W8, int64_t ldw, const float* w_scale,
               void* C, int64_t ldc, const float* bias, const void* R, int64_t ldr, int64_t M, int64_t N, int64_t K,
               int out_dtype, int a_op, vg_stream_t stream);
/* MXFP4 prefill GEMM (cfg prefill_gemm = "mxfp4": the LLM's MLP on the packed rows the decode step streams):
 *   C[m,n] = a_scale[m] * sum_k e4m3(A8[m,k]) * 2^(s[n, k / 32] - 127) * e2m1(W4[n,k])  (+ R[m,n]),
 * fp32 accumulation on v_mfma_scale_f32_32x32x64_f8f6f4 with A = e4m3 (unit scale) and B = e2m1 with the weight's e8m0 byte as its hardware block scale.
 * A8 [M,K] (lda bytes per row) and a_scale [M] are what vg_quantize_fp8_rows produces.  W4 = the PACKED rows of vg_decode_gemv_w4 read in place: row n at
 * W4 + n * ldw_bytes = a head of 64 * SPL scale bytes (byte lane * SPL + u = the scale of block 64 u + lane), then K / 2 code bytes, element 2j in the low
 * nibble of byte j; no second copy of codes or scales is made.  A scale byte 0 means the block is exactly zero whatever its codes hold (as in every
 * MXFP4 entry point).  a_op = 0: N rows of W4, optional residual R of the output dtype; a_op = 1: W4 = [gate; up] = 2N rows and C[m,n] =
 * silu(gate) * up with gate and up rounded to the output dtype first (vg_gemm_f8's SwiGLU), R must be NULL.  out_dtype VG_BF16 | VG_F32; no bias.
 * Shapes: M > 16, K in {3072, 4096, 8192, 14336}, N a multiple of 8 (vg_gemm_w4a8_supported(N, K) != 0, launches nothing), VG_ERR_UNSUPPORTED otherwise.
 * lda and ldw_bytes multiples of 16 that cover a row, A8 / W4 16-byte aligned, C / R rows 16-byte aligned: VG_ERR_ARG otherwise.  No workspace. */
int vg_gemm_w4a8_supported(int64_t N, int64_t K);
int vg_gemm_w4a8(const uint8_t* A8, int64_t lda, const float* a_scale, const uint8_t* W4, int64_t ldw_bytes, void* C, int64_t ldc,
                 const void* R, int64_t ldr, int64_t M, int64_t N, int64_t K, int out_dtype, int a_op, vg_stream_t stream);
/* Which kernel an (M, N, K) GEMM of vg_gemm / vg_gemm_window / vg_gemm_ln is routed to with the current knobs (VG_GEMM_RR, VG_GEMM_P8).  bench.py
 * attributes per-launch times to kernels with it, ops.linear decides its tail split and ops.linear_ln its fused form:
 *   0 gemm_skinny_kernel (M <= 16), 1 gemm_tile_glds_kernel (128x128 tiles, LDS-DMA; its SwiGLU tile form included), 2 gemm_tile_k64b_kernel,
 *   3 gemm_tile_p8_kernel (256x256 tiles, phase-split), 4 gemm_tile_s128_kernel, 5 gemm_small64_kernel, 6 gemm_tile_p8n_kernel (256x192 tiles),
 *   7 gemm_rr_kernel (row-register, K = 144 / 288).
 * The answer is the launcher's own plan (gemm_plan, videoglamm_amd/csrc/vg_gemm_route.h) for the contiguous, 16-byte aligned, batch-1 call without an
 * epilogue: lda = ldw = K, ldc = N, bf16 output for bf16 input and fp32 otherwise, no bias / activation / LayerScale / residual.  A call whose strides,
 * alignment, epilogue or batch differ can be refused by a kernel the query names (vg_gemm_ln then returns VG_ERR_UNSUPPORTED; vg_gemm takes the next kernel
 * of the plan).  N = output columns (F for a_op == 1).
 * windowed != 0: a vg_gemm_window call whose geometry is unknown here, so no 256-row kernel takes its window form and the answer is one of 1, 2, 4, 7.  The
 * launcher itself sends a padding-free gather or scatter of power-of-two windows to kernels 3 / 6 when the shape rules say so: for those calls the
 * answer names the 128x128 kernel that would run otherwise.
 * Launches nothing. */
int vg_gemm_route(int64_t M, int64_t N, int64_t K, int in_dtype, int a_op, int windowed);

/* ---- mask post-processing and evaluation counts: integer / byte work ---- */
/* Connected components of N binary images [N,H,W] (uint8, foreground = nonzero), connectivity 4 or 8.
 * labels: 0 on background, 1 + the smallest linear pixel index (y*W + x) of the component on foreground;
 * counts: area of the pixel's component, 0 on background.  Replaces _C.get_connected_componnets
 * (R/model/segment_anything_2/sam2/csrc/connected_components.cu:213-282, 8-connectivity; called from
 * R/model/segment_anything_2/sam2/utils/misc.py:47-63): same partition and areas; the reference's label VALUES are an
 * artefact of its 2x2-block union-find, only labels > 0 and the areas are consumed (misc.py:223-224).
 * Odd H / W are accepted (the reference asserts even sizes, connected_components.cu:226-227). */
int vg_connected_components(const uint8_t* mask, int32_t* labels, int32_t* counts, int N, int H, int W,
                            int connectivity, vg_stream_t stream);
/* out = mask with every 4-connected component of fewer than min_size pixels cleared (uint8 0/1).
 * remove_small_blobs, R/eval_gcg_infer.py:20-29 (skimage.morphology.remove_small_objects on a bool image).
 * ws_labels / ws_counts: int32 [N,H,W] scratch. */
int vg_remove_small_blobs(const uint8_t* mask, uint8_t* out, int32_t* ws_labels, int32_t* ws_counts, int N, int H,
                          int W, int min_size, vg_stream_t stream);
/* out = scores with every 8-connected background (score <= 0) component of area <= max_area set to 0.1
 * fill_holes_in_mask_scores, R/model/segment_anything_2/sam2/utils/misc.py:216-227 (switched off in the reference's
 * predictor, sam2_video_predictor.py:971-975: a flag on this side too). */
int vg_fill_holes(const float* scores, float* out, int32_t* ws_labels, int32_t* ws_counts, int N, int H, int W,
                  int max_area, vg_stream_t stream);
/* inter[p,g] = |a_p & b_g|, uni[p,g] = |a_p | b_g| over L pixels; a:[P,L], b:[G,L] uint8 (nonzero = set).
 * diagonal != 0 (P == G): only the pairs (i, i), outputs [P] — the per-frame Jaccard of one object.
 * compute_iou R/eval_gcg_metrics.py:26-37; db_eval_iou R/eval_referdavis_metrics.py:147-176 (no void pixels). */
int vg_mask_pair_counts(const uint8_t* a, const uint8_t* b, int64_t* inter, int64_t* uni, int P, int G, int64_t L,
                        int diagonal, vg_stream_t stream);
/* out[n] = {n_fg, n_gt, fg_match, gt_match}: pixels of the two 1-pixel boundary maps (_seg2bmap,
 * R/eval_referdavis_metrics.py:262-305, same-size case) and how many of each lie within the disk of the given radius
 * (skimage disk: dx^2 + dy^2 <= r^2; cv2.dilate border = ignore) of the other one — the integer part of f_measure,
 * R/eval_referdavis_metrics.py:194-259.  fg, gt: uint8 [N,H,W]. */
int vg_boundary_counts(const uint8_t* fg, const uint8_t* gt, int64_t* out, int N, int H, int W, int radius,
                       vg_stream_t stream);
/* The class counts of the validation metrics (gIoU / cIoU) from mask LOGITS, all N masks of a call in one pass:
 * intersectionAndUnionGPU(output = (logit > 0), target, K = 2, ignore_index), R/utils/utils.py:78-90, as the validator
 * calls it per frame (R/utils/trainer.py:443-447).  logits: [N, L] of dtype VG_F32 | VG_BF16, contiguous; target: [N, L]
 * uint8; out: int64 [N, 6] = {inter0, inter1, out0, out1, tgt0, tgt1}.
 *   - the predicted class of a pixel is logit > 0, strictly: 0.0, -0.0, NaN and -inf are class 0, +inf and the smallest
 *     positive denormal are class 1; in bf16 the comparison is on the stored value;
 *   - a pixel whose target equals ignore_index counts in nothing;
 *   - every other pixel counts in out[class]; if its target t is 0 or 1 also in tgt[t], and in inter[t] if class == t;
 *   - so a target value that is neither 0, 1 nor ignore_index counts in out only (histc with min = 0, max = 1 drops it).
 * The union is not an output: the caller forms out + tgt - inter.  Accumulators are int64 and pixel indices 64-bit
 * (L may pass 2^31; L < 2^40); integer sums: the result does not depend on the order of the reduction.  out is fully
 * written by the call (no memset by the caller, no dependence on its previous contents).  The inputs need no alignment
 * beyond their element size: an odd L or an odd row start is legal.  N <= 65535.  VG_ERR_ARG before any launch: a null
 * pointer, N <= 0, L <= 0, a dtype that is neither VG_F32 nor VG_BF16, ignore_index outside 0..255. */
int vg_logit_class_counts(const void* logits, const uint8_t* target, int64_t* out, int N, int64_t L, int dtype,
                          int ignore_index, vg_stream_t stream);
/* out[n] = {xmin, ymin, xmax, ymax, area} (int32 [N,5]) of mask n of mask:[N,H,W] uint8 (foreground = nonzero); the
 * maxima are INCLUSIVE pixel indices, an empty mask gives {W, H, -1, -1, 0}.  The integer part of masks_to_boxes,
 * R/utils/grounding_utils/box_ops.py:118-142.  All N masks in one call; out is fully written by the call (no memset
 * by the caller, no dependence on its previous contents); mask needs no alignment.  Integer min / max / sum: the
 * result does not depend on the order of the reduction.  H * W < 2^31, N <= 65535. */
int vg_mask_boxes(const uint8_t* mask, int32_t* out, int N, int H, int W, vg_stream_t stream);
/* The same table for the mask AFTER vg_remove_small_blobs(min_size) (4-connectivity, components of fewer than
 * min_size pixels cleared), without writing that mask and reading it back: bit for bit
 * vg_mask_boxes(vg_remove_small_blobs(mask, min_size)) — R/eval_grounding.py:281-287.  out_mask: NULL, or uint8
 * [N,H,W] that receives exactly what vg_remove_small_blobs writes.  ws_labels / ws_counts: int32 [N,H,W] scratch.
 * min_size <= 0 is VG_ERR_ARG (vg_mask_boxes is the unfiltered reduction). */
int vg_blob_boxes(const uint8_t* mask, int32_t* out, uint8_t* out_mask, int32_t* ws_labels, int32_t* ws_counts, int N,
                  int H, int W, int min_size, vg_stream_t stream);
/* COCO's uncompressed run-length code of every mask of mask:[N,H,W] uint8 (foreground = nonzero), in the form of
 * mask_to_rle_pytorch (R/model/segment_anything_2/sam2/utils/amg.py:109-137): the pixels in COLUMN-major order
 * j = x * H + y; P = the ascending j >= 1 whose foreground bit differs from that of j - 1 (across column ends too); the
 * counts are the differences of [0] + P + [H * W], with a single 0 in front when pixel 0 is foreground.  An empty mask is
 * [H * W], a full one [0, H * W].  Two phases, so that the caller allocates the output exactly:
 *   vg_mask_rle_count  n_runs[n] (int32 [N]) = len(P) + 1 + fg(pixel 0), and ws_cols (int32 [N, 4, U] scratch, fully
 *                      rewritten by every call; U = vg_mask_rle_units(H, W) = W * ceil(H / R) column segments of
 *                      R = max(64, ceil(H / 65535)) rows) = what the second phase needs per column segment: its write
 *                      offset (the exclusive scan of the segments' transition counts in the code's order), the last
 *                      transition at or before its end (a max-scan), its first / last pixel and whether its first pixel
 *                      opens a run.
 *   vg_mask_rle_emit   offsets: int64 [N + 1], the exclusive sum of n_runs, made by the caller; counts: int32
 *                      [offsets[N]].  Mask n's counts go to counts[offsets[n] : offsets[n + 1]], all of them and nothing
 *                      else; every store index is clamped to that range.  mask and ws_cols as the first phase left them.
 * Each phase reads the mask once, in dwords along the rows (a lane owns 4 adjacent columns and walks down them); stream
 * order is the only dependency between the launches.  mask needs no alignment.  H * W < 2^31, 4 * U < 2^31 (it bites
 * only for masks of at most 64 rows and W >= 2^29), N <= 65535; vg_rle_to_mask refuses the same shapes. */
int vg_mask_rle_units(int H, int W); /* U of ws_cols; 0 for a shape the entry points refuse.  Launches nothing. */
int vg_mask_rle_count(const uint8_t* mask, int32_t* ws_cols, int32_t* n_runs, int N, int H, int W, vg_stream_t stream);
int vg_mask_rle_emit(const uint8_t* mask, const int32_t* ws_cols, const int64_t* offsets, int32_t* counts, int N, int H,
                     int W, vg_stream_t stream);
/* The inverse (rle_to_mask, amg.py:140-151): out:[N,H,W] uint8 0 / 1, row-major, from counts (int32, flat) and offsets
 * (int64 [N + 1], nondecreasing, offsets[N] <= the length of counts: they are read, and trusted).  ws_ends: int32 scratch
 * of the length of counts (the per-mask inclusive scan).  status[n] (int32 [N]) = 1 and mask n all zero when a count of
 * code n is negative or its counts do not sum to exactly H * W; other masks are unaffected.  Zero counts inside a code are
 * legal.  Gather form: every output pixel looks its run up, so no count value takes part in a store address. */
int vg_rle_to_mask(const int32_t* counts, const int64_t* offsets, uint8_t* out, int32_t* status, int32_t* ws_ends, int N,
                   int H, int W, vg_stream_t stream);

/* ---- small MLP heads (r06) ----
 * vg_mlp3_grouped: G independent three-layer MLPs (Linear, ReLU, Linear, ReLU, Linear; sigmoid on the outputs of head g when bit g of sig_mask is set)
 * in one launch: SAM2's output_hypernetworks_mlps (G = 4), iou_prediction_head + pred_obj_score_head (G = 2) and obj_ptr_proj (G = 1) —
 * R/modeling/sam/mask_decoder.py:232-245, R/modeling/sam2_base.py:425-431, MLP = R/modeling/sam2_utils.py:108-132.  bf16 rows and weights.
 *   x: head g reads rows x + g * x_gs + r * x_rs (r < R; strides in elements, multiples of 8), K inputs each.
 *   w0, w1, w2: the heads' nn.Linear weights ([Hd, K], [Hd, Hd], [No, Hd] per head) stacked over the heads and PACKED in MFMA fragment order, so that a wave's
 *   load is one contiguous KiB: [G][ceil(out / 32)][in / 16][64][8] with element (g, t, s, lane, e) = W_g[32 t + lane % 32][16 s + 8 (lane / 32) + e], rows past
 *   `out` zero (videoglamm_amd/ops.py:mlp3_pack is the reference packing).  b0 [G, Hd], b1 [G, Hd], b2 [G, No]: fp32, plain.
 *   out: element (r, g, c) at out + r * o_rs + g * o_gs + c (c < No), out_dtype bf16 or fp32.  K, Hd multiples of 16 in [16, 256], No in [1, 256].
 * The activations between the layers are rounded to bf16, as vg_gemm's bf16 outputs are. */
int vg_mlp3_grouped(const void* x, int64_t x_rs, int64_t x_gs, const void* w0, const float* b0, const void* w1, const float* b1, const void* w2,
                    const float* b2, void* out, int64_t o_rs, int64_t o_gs, int out_dtype, int G, int R, int K, int Hd, int No, unsigned sig_mask,
                    vg_stream_t stream);

/* ---- image pre-processing: uint8 frames in HBM -> the three model inputs ---- */
/* One 8-bit pass of Pillow's separable resampler over in:[N,H,W,C] uint8 (C <= 4): axis 1 resizes W -> out_size
 * (out:[N,H,out_size,C]), axis 0 resizes H -> out_size (out:[N,out_size,W,C]).  bounds:[out_size,2] = (first input
 * index, tap count), coeffs:[out_size,ksize] = 22-bit fixed-point weights (Pillow src/libImaging/Resample.c:
 * precompute_coeffs + normalize_coeffs_8bpc; computed on the host by videoglamm_amd/preproc.py).
 * out = clip8((2^21 + sum_k in[first + k] * coeff[k]) >> 22): bit-exact with PIL.Image.resize — what
 * torchvision's resize(to_pil_image(x), size) runs at R/utils/sam_transforms.py:44-49 and the CLIP processor's
 * bicubic resize at R/utils/enc_preprocessors.py:120-166. */
int vg_resample_u8(const uint8_t* in, uint8_t* out, int N, int H, int W, int C, int out_size, int axis,
                   const int32_t* bounds, const int32_t* coeffs, int ksize, vg_stream_t stream);
/* OpenCV's cv2.resize(img, (Wo, Ho)) with the default INTER_LINEAR on N uint8 images [N,H,W,C] -> [N,Ho,Wo,C]: the InternVideo2
 * stream of the reference's pre-processing (R/model/videogpt_plus/model/internvideo/utils.py:124).  2 taps per axis in 11-bit
 * fixed point (imgproc/src/resize.cpp: HResizeLinear + VResizeLinear with FixedPtCast<int, uchar, 22>), no antialiasing.
 * xi / yi: int32 [Wo,2] / [Ho,2] source indices (already clamped), xa / yb: int32 [Wo,2] / [Ho,2] taps (sum 2048), computed by
 * the host in OpenCV's float32 arithmetic (videoglamm_amd/host.py:cv_linear_taps).  An exact 2x down-scale on both axes takes
 * the INTER_AREA fast path cv::resize re-routes it to ((a+b+c+d+2)>>2; tables may be NULL).  H == Ho && W == Wo is refused. */
int vg_resize_cv_linear_u8(const uint8_t* in, uint8_t* out, int N, int H, int W, int C, int Ho, int Wo, const int32_t* xi,
                           const int32_t* xa, const int32_t* yi, const int32_t* yb, vg_stream_t stream);

/* in:[N,H,W,3] uint8, crop (top,left,h,w) -> out:[N,3,h,w] planar.  mean / std: three doubles each on the HOST.
 * mode 0: fp32 (x - mean) / std on 0..255 values (SAM: R/utils/sam_transforms.py:50-55);
 * mode 1: (x / 255 - mean) / std evaluated in fp64, rounded once (the encoder processors' numpy arithmetic,
 * R/model/videogpt_plus/model/internvideo/utils.py:105-143, R/utils/enc_preprocessors.py:120-166). */
int vg_normalize_u8(const uint8_t* in, void* out, int N, int H, int W, int top, int left, int h, int w,
                    const double* mean, const double* std, int mode, int out_dtype, vg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VG_KERNELS_H */
