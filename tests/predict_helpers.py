"""Helpers shared by the predict_answers tests and tests/golden/make_golden_predict_answers.py, on the fixture model of
tests/generate_helpers.py (fp32 transformers LlamaForCausalLM, CPU): a seeded closed answer set, the literal
answer-ranking procedure of the reference's MSR3D.predict_answers (every candidate as a full copy of prompt + answer
through the whole model), and an fp32 CPU engine with the interface msr3d_amd/llm/generate.py::rank_answers is written
against (prefill / score), built on the same model with its own key / value cache.  CPU only."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

from tests.generate_helpers import CFG, positions_of

BOS, PAD = 1, 0


def answer_set(seed, A=40, S=8, vocab=CFG["vocab"]):
    """-> answer_ids (A, S) int64, answer_mask (A, S) int64: bos, then 1 .. S - 1 real tokens, right-padded with PAD (what
    a tokenizer with padding="longest" on the right returns).  The first real tokens are DISTINCT, so no two answers tie
    in the first-token selection; answer 0 has the full length, answer 1 a single token."""
    rng = np.random.default_rng(seed + 7000)
    first = rng.choice(np.arange(3, vocab), size=A, replace=False)
    n = rng.integers(1, S, size=A)
    n[0], n[1] = S - 1, 1
    ids = np.full((A, S), PAD, np.int64)
    ids[:, 0] = BOS
    ids[:, 1] = first
    for a in range(A):
        ids[a, 2:1 + n[a]] = rng.integers(3, vocab, size=n[a] - 1)
    mask = (np.arange(S)[None] < (1 + n)[:, None]).astype(np.int64)
    return torch.from_numpy(ids), torch.from_numpy(mask)


@torch.no_grad()
def literal_predict_answers(model, x, keep, answer_ids, answer_mask, num_ans_candidates):
    """The reference's procedure, literally.  x (B, T, hidden) ends with the bos embedding (mask 1).
    1. one forward over the prompt (a mask, no position ids); the last position's next-token distribution;
    2. the C answers whose first real token is most probable;
    3. every prompt repeated C times with its bos column cut off, a whole candidate answer (bos included) appended to each
       copy with its padding mask, labels = the answer's real tokens except bos, one forward over all B C sequences,
       the token losses summed per sequence and divided by the number of labelled tokens; the smallest wins.
    -> dict(logits0 (B, V), first_prob (B, A), topk_ids (B, C), loss (B, C), answers_id (B,))."""
    table = model.model.embed_tokens.weight
    B, A, S = x.shape[0], answer_ids.shape[0], answer_ids.shape[1]
    C = min(int(num_ans_candidates), A)
    logits0 = model(inputs_embeds=x, attention_mask=keep).logits[:, -1, :]
    first_prob = F.softmax(logits0, dim=1).index_select(1, answer_ids[:, 1])
    topk_ids = first_prob.topk(C, dim=1)[1]
    cand_ids = answer_ids[topk_ids.reshape(-1)]                      # (B C, S), prompt-major
    cand_mask = answer_mask[topk_ids.reshape(-1)]
    xs = torch.cat([x.repeat_interleave(C, 0)[:, :-1], table[cand_ids]], 1)
    ks = torch.cat([keep.repeat_interleave(C, 0)[:, :-1], cand_mask], 1)
    labels = torch.full(ks.shape, -100, dtype=torch.int64)
    labels[:, -S:] = torch.where(cand_mask.bool(), cand_ids, torch.full_like(cand_ids, -100))
    labels[:, -S] = -100                                             # bos is a condition, not a target
    logits = model(inputs_embeds=xs, attention_mask=ks).logits.float()
    tgt = labels[:, 1:]
    tok = F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), tgt.reshape(-1), reduction="none").view(B * C, -1)
    loss = (tok.sum(1) / (tgt >= 0).sum(1)).view(B, C)
    best = loss.argmin(1)
    return dict(logits0=logits0, first_prob=first_prob, topk_ids=topk_ids, loss=loss,
                answers_id=topk_ids[torch.arange(B), best], sequences=xs, sequences_mask=ks, labels=labels)


class HFScoreEngine:
    """The `prefill` / `score` interface of rank_answers on the fixture's fp32 transformers model (CPU), the twin of
    generate_helpers.HFEngine.  positions="arange" hands transformers a mask and no position ids (slot t rotated by t);
    `force_positions="mask"` overrides that with cumsum(mask) - 1 in both stages -- NOT what the reference computes: it is
    there so that a test can show the difference on a prompt with masked slots inside it."""

    def __init__(self, model, force_positions=None):
        self.model, self.cache, self.mask, self.force = model, None, None, force_positions

    @torch.no_grad()
    def prefill(self, inputs_embeds, attention_mask, positions="mask"):
        from transformers import DynamicCache
        positions = self.force or positions
        self.positions = positions
        self.cache = DynamicCache(config=self.model.config)
        self.mask = attention_mask.long().clone()
        pid = positions_of(self.mask) if positions == "mask" else None
        out = self.model(inputs_embeds=inputs_embeds.float(), attention_mask=self.mask, position_ids=pid,
                         past_key_values=self.cache, use_cache=True)
        return out.logits[:, -1].float()

    @torch.no_grad()
    def score(self, token_embeds, token_keep):
        B, C, S, H = token_embeds.shape
        cache = copy.deepcopy(self.cache)                            # `score` leaves the prefilled cache as it was
        cache.batch_repeat_interleave(C)
        mask = torch.cat([self.mask.repeat_interleave(C, 0), token_keep.reshape(B * C, S).long()], 1)
        pid = positions_of(mask)[:, -S:] if self.positions == "mask" else None
        out = self.model(inputs_embeds=token_embeds.reshape(B * C, S, H).float(), attention_mask=mask, position_ids=pid,
                         past_key_values=cache, use_cache=True)
        return out.logits.view(B, C, S, -1).float()
