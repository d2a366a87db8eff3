"""Several clips, one prompt each (model.inference_clips): every clip runs its own towers and its own whole-prompt prefill — the
launches of vlm.generate() — and then the clips of a group decode together, one row per clip, in the batched step of DESIGN 11.

The evaluation drivers that ask one question per clip, clip after clip (R/eval_gcg_infer.py, R/eval_grounding.py,
R/eval_anet_entities_infer.py) have no prefix to share, but the weight stream of a decode step can still be shared: RowsDecode with row0 = 0
keeps EVERY key / value row of clip b in slot b, so nothing of the step reads the decoder's own cache and that cache is free for the next
clip's prefill while the earlier clips wait for the group's decode.
"""
import os

import torch

from . import ops
from .prompts import BUCKETS, GROUP, batched_route, bucket, decode_rows, rows_cover, sampling_route
from .vlm import IMAGE_TOKEN_INDEX, LlamaDecoder, RowsDecode, generate, splice, stage_mark, wants_scores

BOUND_STEP = 256      # n_bound is rounded up to a multiple of this: groups of similar clips then reuse one RowsDecode and its captured graphs
CLIP_FIELDS = ("images", "context_images", "images_for_sam", "input_ids", "resize_list", "original_size_list")


def groups(n, size=GROUP):
    """[(first, last + 1)] of the consecutive groups n clips run in"""
    return [(g, min(g + size, n)) for g in range(0, n, size)]


def decoder_len(need):
    """the cache length a decoder is made with for `need` rows (vlm.generate's rule)"""
    return -(-need // 1024) * 1024


def slot_bound(lens, max_new_tokens, max_len):
    """n_bound of a group's slots: every position a clip of the group reaches is < max(lens) + max_new_tokens + 1; rounded up to BOUND_STEP and
    kept within the decoder's max_len (the attention kernels and the cos / sin tables end there)"""
    need = max(lens) + max_new_tokens + 1
    if need > max_len:
        raise ValueError(f"a clip of {max(lens)} rows + {max_new_tokens} new tokens does not fit a decoder of {max_len} rows")
    return min(-(-need // BOUND_STEP) * BOUND_STEP, max_len)


def visual_rows(cfg, images, context_images):
    """rows VisionTowers.encode returns for this clip, from the shapes alone (the slots are sized before any tower has run)"""
    pc = cfg["clip"]["patch_size"]
    if context_images is None:
        return images.shape[0] * (images.shape[-2] // pc) * (images.shape[-1] // pc)
    pv = cfg["iv2"]["patch_size"]
    te = images.shape[0]
    return te * ((context_images.shape[-2] // pc // 2) * (context_images.shape[-1] // pc // 2) + (images.shape[-2] // pv // 2) * (images.shape[-1] // pv // 2))


def spliced_rows(input_ids, nvis):
    """rows of vlm.splice(input_ids, visual [nvis, D]): the run of placeholders, first to last, is replaced by the visual block"""
    pos = (input_ids == IMAGE_TOKEN_INDEX).nonzero().flatten()
    if pos.numel() == 0:
        return int(input_ids.numel())
    return int(input_ids.numel()) - (int(pos[-1]) - int(pos[0]) + 1) + int(nvis)


def as_clip(clip, b=0):
    """clip b of inference_clips() as the six arguments of inference(): a tuple / list of six, or a dict with CLIP_FIELDS"""
    if isinstance(clip, dict):
        missing = [k for k in CLIP_FIELDS if k not in clip]
        if missing:
            raise ValueError(f"clips[{b}]: missing {', '.join(missing)}; a clip is the six per-clip arguments of inference(): {', '.join(CLIP_FIELDS)}")
        return tuple(clip[k] for k in CLIP_FIELDS)
    if not isinstance(clip, (tuple, list)) or len(clip) != len(CLIP_FIELDS):
        raise ValueError(f"clips[{b}]: a clip is the six per-clip arguments of inference() ({', '.join(CLIP_FIELDS)}) as a tuple or a dict")
    return tuple(clip)


def generate_clips(params, cfg, towers, clips, max_new_tokens, eos_token_id=None, token_hook=None, samplings=None, traces=None, visuals=None,
                   after_prefill=None, stages=None, before_clip=None):
    """vlm.generate() for B clips.  clips[b] = (images, context_images, input_ids): device frames and host int64 ids [L_b]; visuals[b], when
    given, replaces the towers for clip b (generate(visual=)).  samplings[b]: None (greedy) or clip b's dict(T, k, p, seed); traces[b]: optional
    dict (trace["argmax"]; trace["scores"] = True is replaced by the clip's per-token records as in generate()).  before_clip(b) / after_prefill(b): called before clip b's towers / once its prefill and first token are enqueued.
    stages: when a list, receives the marks "start" and "decode" (vlm.stage_mark) around the whole call.
    -> [(output ids host int64 [L_b + G_b], pred_embeddings device [N_b, 256])] per clip: exactly generate()'s result for that clip.

    Per clip, in list order: the towers, the splice and ONE prefill of the whole prompt on the decoder (generate()'s launches and shapes, so
    the rows are its bits), the first token, then the clip's K / V rows [0, S_b) and final-norm rows move into slot b of a RowsDecode with
    row0 = 0.  The group then decodes one batched step per token (prompts.decode_rows: per-row EOS, per-row hook step numbering).  More than
    16 clips run as consecutive groups of 16.  A group that prompts.batched_route refuses (one clip, fp32, shapes the B-row kernels do not
    cover, mixed sampling routes, VG_CLIPS_BATCHED=0, ...) is a plain loop of generate(); only a bf16 GPU model whose widths the B-row kernels
    do not cover gets its decoder from here first (sized for the group's longest clip: the route's shape rules are read off the decoder)."""
    B = len(clips)
    samplings = list(samplings) if samplings is not None else [None] * B
    assert len(samplings) == B and (visuals is None or len(visuals) == B) and (traces is None or len(traces) == B)
    out = []
    stage_mark(stages, "start")
    for g0, g1 in groups(B):
        out += _group(params, cfg, towers, clips, g0, g1, max_new_tokens, eos_token_id, token_hook, samplings, traces, visuals, after_prefill,
                      before_clip)
    stage_mark(stages, "decode")
    return out


def _alone(params, cfg, towers, clips, g0, g1, max_new_tokens, eos_token_id, token_hook, samplings, traces, visuals, after_prefill, before_clip):
    res = []
    for b in range(g0, g1):
        images, context_images, ids = clips[b]
        if before_clip is not None:
            before_clip(b)
        res.append(generate(params, cfg, towers, images, context_images, ids, max_new_tokens, eos_token_id,
                            visual=None if visuals is None else visuals[b], token_hook=token_hook,
                            after_prefill=None if after_prefill is None else (lambda b=b: after_prefill(b)),
                            trace=None if traces is None else traces[b], sampling=samplings[b]))
    return res


def _group(params, cfg, towers, clips, g0, g1, max_new_tokens, eos_token_id, token_hook, samplings, traces, visuals, after_prefill, before_clip):
    args = (params, cfg, towers, clips, g0, g1, max_new_tokens, eos_token_id, token_hook, samplings, traces, visuals, after_prefill, before_clip)
    n = g1 - g0
    # what needs no decoder first: the group's size, the switches, one sampling route, and a bf16 model on the GPU (every B-row kernel is bf16)
    vocab = params.t("lm_head.weight").shape[0]
    routes = [sampling_route(samplings[b], vocab) for b in range(g0, g1)]
    dw = cfg["llm"].get("decode_weights")
    if (max_new_tokens <= 1 or params.device.type != "cuda" or params.dtype != torch.bfloat16
            or not batched_route(n, True, dw, 0, routes, os.environ, w8_rows=True, w4_rows=True, switch="VG_CLIPS_BATCHED")):
        return _alone(*args)
    # every clip's spliced length, from the shapes: the decoder and the slots are sized before the first prefill
    lens = []
    for b in range(g0, g1):
        images, context_images, ids = clips[b]
        nvis = visuals[b].shape[0] if visuals is not None and visuals[b] is not None else visual_rows(cfg, images, context_images)
        lens.append(spliced_rows(ids, nvis))
    need = max(lens) + max_new_tokens + 1
    # the shapes the B-row kernels cover are the decoder's to say (rope path, chained launch, fused widths): it is made, or grown, for the group's
    # longest clip here — for a bf16 GPU model of widths the kernels do not cover too, whose loop of generate() then runs on this decoder
    dec = getattr(params, "_decoder", None)
    if dec is None or dec.max_len < need:
        dec = LlamaDecoder(params, cfg["llm"], decoder_len(need))
        params._decoder = dec          # the same cache (and captured decode graphs) generate() uses
    dec.check_dense(cfg["llm"])
    rope_rows, cover = rows_cover(params, dec)
    if not batched_route(n, rope_rows, dw, dec.chain_roles, routes, os.environ, switch="VG_CLIPS_BATCHED", **cover):
        return _alone(*args)
    n_bound = slot_bound(lens, max_new_tokens, dec.max_len)
    key = (bucket(n), 0, n_bound)
    rows = dec.__dict__.setdefault("_rows", {}).get(key)
    if rows is None:
        dec._rows.clear()              # one batched state per decoder
        rows = dec._rows[key] = RowsDecode(dec, bucket(n), 0, n_bound)
    rows.route = routes[0]
    scores = traces is not None and any(wants_scores(traces[b]) for b in range(g0, g1))
    dec.set_scores(scores)
    rows.set_scores(scores)
    seg_idx = cfg["seg_token_idx"]
    eos = set() if eos_token_id is None else ({int(eos_token_id)} if isinstance(eos_token_id, int) else {int(e) for e in eos_token_id})
    ids_out, added = [], []
    for j, b in enumerate(range(g0, g1)):
        images, context_images, ids = clips[b]
        if before_clip is not None:
            before_clip(b)
        visual = visuals[b] if visuals is not None and visuals[b] is not None else towers.encode(images, context_images, None)
        x = splice(params, ids, visual)
        S = x.shape[0]
        if S != lens[j]:
            raise RuntimeError(f"clips[{b}]: the towers returned {visual.shape[0]} visual rows, {S} spliced rows where the shapes said {lens[j]}")
        dec.reset()
        dec.set_sampling(samplings[b])
        hidden = dec.forward(x)[-1:]       # the whole prompt in one prefill: generate()'s launches, so generate()'s bits
        dec.next_token(hidden)
        rows.load_row(j, 0, S)             # K / V rows [0, S) and every final-norm row a [SEG] inside the prompt can need: slot j
        added.append(S - ids.numel())
        ids_out.append(ids.tolist())
        if after_prefill is not None:
            after_prefill(b)
    for j in range(n, rows.B):
        rows.pad_row(j, 0)                 # bucket padding: a row at position 0 of its own slot (one key), its tokens ignored
    decode_rows(rows, ids_out, max_new_tokens, eos, token_hook, None if traces is None else traces[g0:g1])
    res = []
    for j, out_j in enumerate(ids_out):
        # the row of a [SEG] at output position i is i - 1 + added (generate()): all of clip j's rows are in slot j
        seg_rows = [i - 1 + added[j] for i in range(1, len(out_j)) if out_j[i] == seg_idx]
        out_ids = torch.tensor(out_j, dtype=torch.int64)
        if not seg_rows:
            res.append((out_ids, torch.empty(0, 256, dtype=params.dtype, device=params.device)))
            continue
        # text_hidden_fcs per clip: the GEMMs see the rows they see when the clip runs alone
        h = rows.rows_of(j, 0, seg_rows)
        fc = "model.text_hidden_fcs.0."
        h = ops.linear(h, params.w(fc + "0"), params.b(fc + "0"), act=ops.ACT_RELU)
        res.append((out_ids, ops.linear(h, params.w(fc + "2"), params.b(fc + "2"))))
    return res
