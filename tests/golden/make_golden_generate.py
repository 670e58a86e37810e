"""Golden vectors for `generate` (msr3d_amd/llm/generate.py), made on the CPU in float32 by transformers'
`LlamaForCausalLM.generate(inputs_embeds=..., attention_mask=..., do_sample=False, ...)` with eager attention, peft's LoRA
formula on all seven projections and the weights of tests/helpers.py::llama_stack_weights (2 layers, hidden 512, 8 heads,
vocab 1024) plus a seeded bf16-rounded embedding table (tests/generate_helpers.py).  The installed transformers (5.x) is
the arbiter; it is asked for `max_new_tokens` / `min_new_tokens`, because given embeddings it subtracts the prompt's
length from `max_length` and `min_length`, while this library counts generated tokens, as the reference's call means it.

    python tests/golden/make_golden_generate.py            # the teacher-forcing fixtures, seed 0
    python tests/golden/make_golden_generate.py gap        # + the free-running fixture (seed search)
    python tests/golden/make_golden_generate.py longpad    # + the long-prompt fixture

generate_seed0_greedy.npz, generate_seed0_greedy_rep.npz (repetition_penalty 3.0): 3 prompts x 24 positions (row 0
unpadded, row 1 left-padded, row 2 with masked slots INSIDE the prompt, the last column the bos embedding), 24 new tokens:
inputs, masks, the sequences and per step the raw logits (and, with the penalty, the processed scores).
generate_seed0_beam5.npz: num_beams 5, repetition_penalty 3.0, 10 new tokens: per step the raw logits of all 15 running
beams, transformers' returned sequences and beam_indices, and the tokens / flat beam indices FED to every step.
transformers returns only the winning hypotheses' history, so the running beams are re-derived here from its per-step
processed scores by its own selection rule; the derivation is checked twice before anything is written: its finished
hypotheses equal transformers' returned sequences, and a teacher-forced fp32 run fed with the derived tokens and beam
indices reproduces transformers' raw logits of every step to 1e-4.  (Its processed scores are in
generate_seed0_beam5_scores.npz: one file would exceed the size limit of a committed file.)

generate_longpad_seed0.npz: greedy, 8 new tokens on 3 prompts x 200 positions: row 1 left-padded by 140 (two whole 64-key
blocks of the attention kernels and part of the third), row 2 with the slots 150 .. 174 masked inside the prompt; the
prefill crosses three blocks of the cache, the decode steps start at length 200.

generate_gap_seed<S>.npz: the free-running case -- 2 prompts (row 1 left-padded) x GAP_STEPS new tokens, greedy with
repetition_penalty 3.0, from a seed whose EVERY step has a decision margin of at least M_GAP.  The margin of a
step is min over the other tokens j of (s_top - s_j) / max(a_top, a_j), s the processed scores and a the factor by
which the processor multiplies an error of the raw logit (the penalty for a penalised negative logit, 1 otherwise): two
raw-logit vectors closer than margin / 2 to the reference in every entry pick the same token.

M_GAP = 4 x the largest absolute deviation of the PARENT commit's LoRALlamaStack.logits (the full forward, existing code)
from generate_seed0_greedy.npz's fp32 logits on the same prefixes, rows 0 and 1 (row 2's masked slots inside the prompt
are where the full forward's arange positions legitimately differ), measured once on an MI355X: see MEASURED_PARENT_DEV.
The factor 4 covers the cached path's different summation order.
With 8 new tokens no seed searched reaches M_GAP = 0.179 (SEARCHED below: the best smallest margin is 0.165), so the case is
shortened to 6 tokens rather than the margin lowered: seed 2919 has a smallest margin of 0.273 over its 6 steps.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.generate_helpers import CFG, HFEngine, embed_table, hf_generate, hf_model, prompt  # noqa: E402

MEASURED_PARENT_DEV = 0.044699907302856445          # rows 0 and 1, 24 steps each (logits of unit spread); row 2: 1.49
M_GAP = 4 * MEASURED_PARENT_DEV
REP = 3.0
EOS = PAD = 2
GAP_STEPS, GAP_SEED = 6, 2919
SEARCHED = "8 tokens: seeds 0-2399 all, 2400-5599 in part: best smallest margin 0.165 (seed 3215); 6 tokens: seed 2919, 0.273"


def _cfg_rec(seed):
    c = CFG
    return {"cfg": np.array([c[k] for k in ("layers", "hidden", "heads", "inter", "vocab", "r", "alpha")], np.int64),
            "eps": np.float64(c["eps"]), "theta": np.float64(c["theta"]), "seed": np.int64(seed)}


def _save(name, rec):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < (1 << 20), (name, size)
    print(path, size, "bytes")


def greedy_fixture(seed, model, x, keep, rep, name, steps=24):
    out = hf_generate(model, x, keep, steps, repetition_penalty=rep, eos_id=EOS, pad_id=PAD, full=True)
    rec = dict(_cfg_rec(seed), x=x.numpy(), keep=keep.numpy().astype(np.uint8), sequences=out.sequences.numpy(),
               logits=torch.stack(out.logits).numpy(), repetition_penalty=np.float64(rep), eos=np.int64(EOS))
    if rep != 1.0:
        rec["scores"] = torch.stack(out.scores).numpy()
    assert out.sequences.shape[1] == steps and not (out.sequences == EOS).any(), "an early eos: pick another seed"
    _save(name, rec)


def beam_fixture(seed, model, x, keep, nb=5, steps=10):
    out = hf_generate(model, x, keep, steps, num_beams=nb, repetition_penalty=REP, eos_id=EOS, pad_id=PAD, full=True)
    B, V, K2 = x.shape[0], CFG["vocab"], 2 * nb
    scores = torch.stack(out.scores)                       # (S, B nb, V): processors(log_softmax(logits))
    S = scores.shape[0]
    run = torch.zeros(B, nb)
    run[:, 1:] = -1.0e9
    offs = (torch.arange(B) * nb)[:, None]
    feed_tok, feed_idx = [], []
    for s in range(S):
        acc = (scores[s].view(B, nb, V) + run[:, :, None]).view(B, nb * V)
        val, idx = torch.topk(acc, K2)
        src, tok = idx // V, idx % V
        hits = (tok == EOS) | (s + 1 >= steps)
        lp = val + hits.float() * -1.0e9
        nxt = torch.topk(lp, nb)[1]
        run = lp.gather(1, nxt)
        feed_tok.append(tok.gather(1, nxt).reshape(-1))
        feed_idx.append((src.gather(1, nxt) + offs).reshape(-1))
    feed_tok, feed_idx = torch.stack(feed_tok), torch.stack(feed_idx)
    # check 1: a teacher-forced fp32 run fed with the derived beams reproduces transformers' raw logits
    emb = torch.from_numpy(embed_table(seed))
    eng = HFEngine(model)
    lg = eng.prefill(x, keep).repeat_interleave(nb, 0)
    eng.expand(nb)
    worst = 0.0
    for s in range(S):
        worst = max(worst, float((lg - out.logits[s]).abs().max()))
        if s + 1 < S:
            lg = eng.step(emb[feed_tok[s]], feed_idx[s])
    assert worst < 1e-4, worst
    # check 2: the search this library runs on that engine returns transformers' sequences
    from msr3d_amd.llm.generate import search
    mine = search(HFEngine(model), lambda ids: emb[ids], x, keep, eos_id=EOS, pad_id=PAD, num_beams=nb, max_length=steps,
                  min_length=0, repetition_penalty=REP, length_penalty=1.0)
    assert torch.equal(mine, out.sequences)
    rec = dict(_cfg_rec(seed), x=x.numpy(), keep=keep.numpy().astype(np.uint8), sequences=out.sequences.numpy(),
               beam_indices=out.beam_indices.numpy(), logits=torch.stack(out.logits).numpy(),
               feed_tokens=feed_tok[:S - 1].numpy(), feed_beam_idx=feed_idx[:S - 1].numpy(), num_beams=np.int64(nb),
               repetition_penalty=np.float64(REP), eos=np.int64(EOS), teacher_forced_dev=np.float64(worst))
    _save(f"generate_seed{seed}_beam{nb}.npz", rec)
    _save(f"generate_seed{seed}_beam{nb}_scores.npz", {"scores": scores.numpy(), "seed": np.int64(seed)})


def margins(logits, scores, prev, rep):
    """logits, scores (B, V) of one step, prev (B, n) the generated tokens -> (B,) decision margins (module docstring)."""
    amp = torch.ones_like(logits)
    if prev.shape[1]:
        pen = torch.zeros_like(logits, dtype=torch.bool).scatter(1, prev, True)
        amp = torch.where(pen & (logits < 0), torch.full_like(logits, rep), amp)
    top, it = scores.max(1, keepdim=True)
    d = (top - scores) / torch.maximum(amp, amp.gather(1, it))
    d.scatter_(1, it, float("inf"))
    return d.min(1)[0]


def gap_fixture(m_gap, seeds=range(GAP_SEED, GAP_SEED + 1), steps=GAP_STEPS):
    for seed in seeds:
        model = hf_model(seed)
        x, keep = prompt(seed, B=2)
        out = hf_generate(model, x, keep, steps, repetition_penalty=REP, eos_id=EOS, pad_id=PAD, full=True)
        if out.sequences.shape[1] != steps or (out.sequences == EOS).any():
            continue
        gaps = torch.stack([margins(out.logits[s], out.scores[s], out.sequences[:, :s], REP) for s in range(steps)])
        print(seed, float(gaps.min()), flush=True)
        if float(gaps.min()) >= m_gap:
            rec = dict(_cfg_rec(seed), x=x.numpy(), keep=keep.numpy().astype(np.uint8), sequences=out.sequences.numpy(),
                       logits=torch.stack(out.logits).numpy(), gaps=gaps.numpy(), m_gap=np.float64(m_gap),
                       parent_dev=np.float64(MEASURED_PARENT_DEV), searched=np.array(SEARCHED), repetition_penalty=np.float64(REP), eos=np.int64(EOS))
            _save(f"generate_gap_seed{seed}.npz", rec)
            return seed
    raise SystemExit("no seed reaches the margin: search more seeds or shorten the case (never lower M_GAP)")


LONGPAD = dict(B=3, T=200, left_pad=140, hole=(150, 175))


def longpad_fixture(seed=0, steps=8):
    model = hf_model(seed)
    x, keep = prompt(seed, **LONGPAD)
    greedy_fixture(seed, model, x, keep, 1.0, f"generate_longpad_seed{seed}.npz", steps=steps)


def main(seed=0):
    model = hf_model(seed)
    x, keep = prompt(seed)
    greedy_fixture(seed, model, x, keep, 1.0, f"generate_seed{seed}_greedy.npz")
    greedy_fixture(seed, model, x, keep, REP, f"generate_seed{seed}_greedy_rep.npz")
    beam_fixture(seed, model, x, keep)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "gap":
        gap_fixture(M_GAP)
    elif len(sys.argv) > 1 and sys.argv[1] == "longpad":
        longpad_fixture(0)
    else:
        main(0)
