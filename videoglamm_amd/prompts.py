"""Several prompts about one clip (model.inference_prompts): the towers, the projectors and the prefill of the shared prefix
run once, then every prompt continues from that prefix.

The shared prefix of a prompt is everything up to and including its visual block: apply_for_chat puts the system text and the
<image> placeholders before the question (R/model/videogpt_plus/conversation.py, R/chat.py), so the evaluation drivers that ask
several questions about one clip (R/eval_referdavis_infer.py:143-205, R/eval_mevis.py:121-160) repeat ~99 % of the prefill rows.
The prefix is a property of each prompt, never of the batch (no common-prefix search): a prompt's prefill splits at the same row
whatever it is batched with, so its arithmetic does not depend on the other prompts.
"""
import os

import torch

from . import ops
from .vlm import IMAGE_TOKEN_INDEX, LlamaDecoder, RowsDecode, decode_loop, read_scores, splice, stage_mark, wants_scores

GROUP = 16       # prompts per pass; longer lists run in consecutive groups
BUCKETS = (2, 4, 8, 16)     # rows of a captured batched decode step


def bucket(B):
    """the captured batched step that runs B prompts: the smallest bucket >= B"""
    for n in BUCKETS:
        if B <= n:
            return n
    raise ValueError(f"{B} prompts: a batched decode step runs at most {BUCKETS[-1]}")


def sampling_route(sampling, vocab):
    """"greedy", "sample_fast" or "sample": the launches a prompt's decode step captures (LlamaDecoder.set_sampling)"""
    if sampling is None:
        return "greedy"
    return "sample_fast" if ops.sample_fast_route(int(sampling["k"]), vocab) else "sample"


def batched_route(B, rope_path, decode_weights, chain, routes, env, attn_rows=False, w8_rows=False, w4_rows=False, switch="VG_PROMPTS_BATCHED"):
    """True when a group of B prompts decodes in one batched step (RowsDecode) instead of one after another.  rope_path: the decoder runs the
    bf16 head_dim-128 rope step (LlamaDecoder.rope_path; B-row kernels cover the shape); attn_rows: the decoder runs the decode_attention step
    (Phi-3-mini width) and the B-row kernels cover its shape (ops.decode_step_rows_supported); decode_weights: cfg["decode_weights"] ("fp8" takes
    the batched step only with w8_rows: the B-row fp8 GEMV covers this decoder's MLP and lm_head row lengths; "mxfp4" only with w4_rows: the B-row MXFP4 GEMV covers the MLP's row lengths and the B-row fp8 GEMV the lm_head's;
    model.inference_prompts() reaches this route for an mxfp4 model with shared=True only); chain: VG_DECODE_CHAIN roles; routes: the set of the prompts' sampling routes; env: the environment (VG_PROMPTS_BATCHED=0 forces the sequential loop;
    VG_DECODE_AHEAD=1 keeps it too); switch: the environment variable whose value "0" forces the sequential loop (clips.generate_clips passes
    VG_CLIPS_BATCHED).  Pure: no device work."""
    return (B >= 2 and B <= BUCKETS[-1] and (bool(rope_path) or bool(attn_rows)) and (decode_weights != "fp8" or bool(w8_rows)) and (decode_weights != "mxfp4" or bool(w4_rows))
            and not chain and len(set(routes)) == 1
            and env.get(switch, "1") != "0" and env.get("VG_DECODE_AHEAD", "0") != "1")


def slot_layout(P, kw, need):
    """(row0, n_bound): slot rows start at the key block that holds position P (row0 = floor(P / kw) * kw, so a key block is wholly shared or
    wholly per slot) and end at `need` (every position a prompt of the group reaches is < need)"""
    row0 = (P // kw) * kw
    assert need > P >= row0
    return row0, need


def prefix_len(input_ids, b=0):
    """input_ids host int64 [L] -> the number of ids up to and including the last visual placeholder (-200)."""
    pos = (input_ids == IMAGE_TOKEN_INDEX).nonzero().flatten()
    if pos.numel() == 0:
        raise ValueError(f"input_ids_list[{b}] has no visual placeholder ({IMAGE_TOKEN_INDEX}): it shares no prefix with the clip")
    return int(pos[-1]) + 1


def check_prompts(ids_list):
    """ValueError naming the first prompt whose ids before the end of the visual block differ from prompt 0's, or that has no placeholder."""
    n0 = prefix_len(ids_list[0], 0)
    head = ids_list[0][:n0]
    for b, ids in enumerate(ids_list[1:], 1):
        n = prefix_len(ids, b)
        if n != n0 or not torch.equal(ids[:n], head):
            raise ValueError(f"input_ids_list[{b}]: the ids up to the end of the visual block differ from input_ids_list[0]'s; "
                             "inference_prompts() needs one shared prefix (system text + visual block) for every prompt")


def generate_prompts(params, cfg, towers, images, context_images, ids_list, max_new_tokens, eos_token_id=None, token_hook=None,
                     samplings=None, traces=None, after_prefix=None, stages=None):
    """vlm.generate() for B prompts on one clip.  ids_list: host int64 [L_b] each, with an identical prefix up to the visual block
    (check_prompts).  samplings[b]: None (greedy) or prompt b's dict(T, k, p, seed); traces[b]: optional dict per prompt (trace["argmax"];
    trace["scores"] = True is replaced by the prompt's per-token records as in generate(), on the batched and on the sequential route).
    after_prefix: called once the prefix is prefilled (VG_HIERA_START=prefill); stages: generate()'s per-stage marks (towers, prefill, decode).
    -> (output ids host int64 [L_b + G_b] per prompt, pred_embeddings device [sum N_b, 256] in prompt order, N_b per prompt).

    Rows [0, P) of the spliced sequence are prefilled once into the decoder's KV cache; every prompt then resumes at position P: its suffix
    [P, S_b) is prefilled on top of the prefix rows and it decodes until its own EOS or max_new_tokens.  A prompt never writes below P, so the
    prefix's K/V and final-norm rows stay valid for the next one; a prompt's own [SEG] rows go through text_hidden_fcs before the next prompt overwrites them."""
    B = len(ids_list)
    samplings = samplings or [None] * B
    seg_idx = cfg["seg_token_idx"]
    eos = set() if eos_token_id is None else ({int(eos_token_id)} if isinstance(eos_token_id, int) else {int(e) for e in eos_token_id})
    stage_mark(stages, "start")
    visual = towers.encode(images, context_images, None)
    stage_mark(stages, "towers")
    n0 = prefix_len(ids_list[0])
    prefix = splice(params, ids_list[0][:n0], visual)
    P = prefix.shape[0]                # spliced rows up to and including the visual block
    table = params.t("model.embed_tokens.weight")
    need = P + max(ids.numel() for ids in ids_list) - n0 + max_new_tokens + 1
    dec = getattr(params, "_decoder", None)
    if dec is None or dec.max_len < need:
        dec = LlamaDecoder(params, cfg["llm"], -(-need // 1024) * 1024)
        params._decoder = dec          # the same cache (and captured decode graphs) generate() uses
    dec.check_dense(cfg["llm"])
    dec.reset()
    dec.forward(prefix)                # K/V and final-norm rows [0, P): shared by every prompt
    stage_mark(stages, "prefill")
    if after_prefix is not None:
        after_prefix()
    vocab = params.t("lm_head.weight").shape[0]
    routes = [sampling_route(sp, vocab) for sp in samplings]
    rope_rows, cover = rows_cover(params, dec)
    batched = max_new_tokens > 1 and batched_route(B, rope_rows, cfg["llm"].get("decode_weights"), dec.chain_roles, routes, os.environ, **cover)
    rows = None
    if batched:
        row0, n_bound = slot_layout(P, dec.kpw2 if dec.rope_path else RowsDecode.ATTN_KW, need)
        key = (bucket(B), row0, n_bound)
        rows = dec.__dict__.setdefault("_rows", {}).get(key)
        if rows is None:
            dec._rows.clear()          # one batched state per decoder: its slots are sized by the clip
            rows = dec._rows[key] = RowsDecode(dec, bucket(B), row0, n_bound)
        rows.route = routes[0]
    scores = any(wants_scores(t) for t in (traces or []))
    dec.set_scores(scores)
    if rows is not None:
        rows.set_scores(scores)
    out, embs, counts = [], [], []
    added = P - n0                     # "num_newly_added_tokens" (VideoGLaMM.py:613,786)

    def take(b, out_b):
        # the row of a [SEG] at output position j is j - 1 + added (generate()); rows >= P belong to prompt b: the sequential loop takes them
        # before the next prompt overwrites them, the batched one reads them from slot b
        seg_rows = [j - 1 + added for j in range(1, len(out_b)) if out_b[j] == seg_idx]
        if seg_rows:
            # text_hidden_fcs per prompt: the GEMMs then see the same rows whether the prompt runs alone or in a batch
            h = rows.rows_of(b, P, seg_rows) if rows is not None else dec.hid_all[torch.tensor(seg_rows, device=params.device)]
            fc = "model.text_hidden_fcs.0."
            h = ops.linear(h, params.w(fc + "0"), params.b(fc + "0"), act=ops.ACT_RELU)
            embs.append(ops.linear(h, params.w(fc + "2"), params.b(fc + "2")))
        counts.append(len(seg_rows))
        return torch.tensor(out_b, dtype=torch.int64)

    for b, ids in enumerate(ids_list):
        dec.reset()
        dec.pos = P
        dec.pos_dev.fill_(P)
        dec.set_sampling(samplings[b])
        # an empty suffix takes its first token from the prefix's last row
        hidden = dec.forward(ops.embed(ids[n0:].to(params.device), table))[-1:] if ids.numel() > n0 else dec.hid_all[P - 1:P]
        out_b = ids.tolist()
        if max_new_tokens > 0:
            dec.next_token(hidden)
        if rows is not None:
            rows.load_row(b, P, P + ids.numel() - n0)      # the decode waits for the whole group
            out.append(out_b)
            continue
        decode_loop(params, dec, out_b, max_new_tokens, eos, token_hook, None if traces is None else traces[b])
        out.append(take(b, out_b))
    if rows is not None:
        for b in range(B, rows.B):
            rows.pad_row(b, P)
        decode_rows(rows, out, max_new_tokens, eos, token_hook, traces)
        out = [take(b, out_b) for b, out_b in enumerate(out)]
    stage_mark(stages, "decode")
    if not embs:
        return out, torch.empty(0, 256, dtype=params.dtype, device=params.device), counts
    return out, torch.cat(embs), counts


def rows_cover(params, dec):
    """(rope_rows, dict(attn_rows, w8_rows, w4_rows)): which forms of the B-row step cover this decoder — batched_route's shape arguments"""
    rope_rows = dec.rope_path and ops.decode_rows_supported(dec.H, dec.Hkv, dec.hd, dec.D, dec.ffn, params.dtype)
    attn_rows = (not dec.rope_path and dec.fused_decode and params.device.type == "cuda"
                 and ops.decode_step_rows_supported(dec.H, dec.Hkv, dec.hd, dec.D, dec.ffn, params.dtype))
    # fp8 / mxfp4 decode weights: every quantised weight of the step (dec.proj: gate|up, down, the lm_head) has a B-row kernel of its shape
    quant = all(dec.proj.covered(N, K, fmt) for N, K, fmt, _ in dec.proj.weights(quantised=True))
    w8_rows, w4_rows = dec.w8 and quant, dec.w4 and quant
    return rope_rows, dict(attn_rows=attn_rows, w8_rows=w8_rows, w4_rows=w4_rows)


def decode_rows(rows, out, max_new_tokens, eos, token_hook=None, traces=None):
    """decode_loop for the live rows of a batched step: per step the B tokens come back in one copy; each prompt applies token_hook with its own step
    numbering (all prompts start together, so that is the loop's step), records trace["argmax"], appends, and retires at an id of `eos` or at
    max_new_tokens; replaced tokens go back in one copy; the step is replayed while any prompt is live."""
    B = len(out)
    live = [True] * B
    n_prompt = [len(o) for o in out]
    for step in range(max_new_tokens):
        toks = rows.tok.cpu().tolist()
        repl_any = False
        for b in range(B):
            if not live[b]:
                continue
            nxt = int(toks[b])
            if traces is not None and traces[b] is not None:
                traces[b].setdefault("argmax", []).append(nxt)
            if token_hook is not None:
                repl = token_hook(step, nxt)
                if repl is not None and int(repl) != nxt:
                    nxt = int(repl)
                    toks[b] = nxt
                    repl_any = True
            out[b].append(nxt)
            if nxt in eos or step == max_new_tokens - 1:
                live[b] = False
        if not any(live):
            break
        if repl_any:
            rows.tok.copy_(torch.tensor(toks, dtype=torch.int64))
        rows.decode_step()
    want = [b for b in range(B) if traces is not None and wants_scores(traces[b])]
    if want:      # one read after the loop; every row is cut to the tokens it emitted itself
        G = [len(out[b]) - n_prompt[b] for b in range(B)]
        sc, t2 = rows.score_hist[:B, :max(G)].cpu(), rows.top2_hist[:B, :max(G)].cpu()
        for b in want:
            traces[b]["scores"] = read_scores(sc[b], t2[b], G[b])
