"""Several prompts about one clip (model.inference_prompts): the towers, the projectors and the prefill of the shared prefix
run once, then every prompt continues from that prefix.

The shared prefix of a prompt is everything up to and including its visual block: apply_for_chat puts the system text and the
<image> placeholders before the question (R/model/videogpt_plus/conversation.py, R/chat.py), so the evaluation drivers that ask
several questions about one clip (R/eval_referdavis_infer.py:143-205, R/eval_mevis.py:121-160) repeat ~99 % of the prefill rows.
The prefix is a property of each prompt, never of the batch (no common-prefix search): a prompt's prefill splits at the same row
whatever it is batched with, so its arithmetic does not depend on the other prompts.
"""
import torch

from . import ops
from .vlm import IMAGE_TOKEN_INDEX, LlamaDecoder, decode_loop, splice, stage_mark

GROUP = 16       # prompts per pass; longer lists run in consecutive groups


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
    (check_prompts).  samplings[b]: None (greedy) or prompt b's dict(T, k, p, seed); traces[b]: optional dict per prompt (trace["argmax"]).
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
    dec.reset()
    dec.forward(prefix)                # K/V and final-norm rows [0, P): shared by every prompt
    stage_mark(stages, "prefill")
    if after_prefix is not None:
        after_prefix()
    out, embs, counts = [], [], []
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
        decode_loop(params, dec, out_b, max_new_tokens, eos, token_hook, None if traces is None else traces[b])
        added = P - n0                 # "num_newly_added_tokens" (VideoGLaMM.py:613,786)
        # the row of a [SEG] at output position j is j - 1 + added (generate()); rows >= P belong to this prompt and are taken now
        rows = [j - 1 + added for j in range(1, len(out_b)) if out_b[j] == seg_idx]
        if rows:
            # text_hidden_fcs per prompt: the GEMMs then see the same rows whether the prompt runs alone or in a batch
            h = dec.hid_all[torch.tensor(rows, device=params.device)]
            fc = "model.text_hidden_fcs.0."
            h = ops.linear(h, params.w(fc + "0"), params.b(fc + "0"), act=ops.ACT_RELU)
            embs.append(ops.linear(h, params.w(fc + "2"), params.b(fc + "2")))
        counts.append(len(rows))
        out.append(torch.tensor(out_b, dtype=torch.int64))
    stage_mark(stages, "decode")
    if not embs:
        return out, torch.empty(0, 256, dtype=params.dtype, device=params.device), counts
    return out, torch.cat(embs), counts
