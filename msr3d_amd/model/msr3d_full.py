"""The full MSR3D training forward, from `obj_fts` to `loss (B,)`: the hot path joined to the language model
(/root/reference/model/msr3d/msr3d.py:274-287 prompter -> llm_proj -> indexed write into `inputs_embeds`,
:378-392 answer tokens appended and targets built, :409-415 LLM forward from `inputs_embeds` + `attention_mask`,
:426-441 per-sequence mean cross-entropy).

    scene dict ─► MSR3DHotPath (visual_prompter + llm_proj)                 ─► scene_embeds (B, L, E) fp32
    input_ids | output_ids ─► embed_tokens (frozen, bf16)                     ─► inputs_embeds (B, T, E) bf16
                 project_scatter_images_train_ (optional: `image_tokens`)     ─► inputs_embeds (image placeholder rows)
                 scatter_scene_embeds_train_ (placeholder rows, mask rows)    ─► inputs_embeds, attention_mask
                 LoRALlamaStack (n decoder layers + norm + head) + seq-CE     ─► loss (B,)

What is NOT here (out of SURVEY §8's scope): tokenizer and prompt assembly (the step takes
token ids), the frozen 2D image backbone (`image_encoder`: ConvNeXt under no_grad, its pooled output is cacheable and comes in as
`img_fts`), CLIP fusion, and of the reference's `generate` only `pred_action`.
The 2D image branch from the backbone's pooled output on (msr3d.py:98-100 `llm_proj_img`, :233-252) is opt-in through
`cfg.image_tokens` (msr3d_amd/model/image_tokens.py): the projected feature of every real image replaces the embedding of one
image placeholder before the scene tokens go in, in training, `generate` and `predict_answers` alike.
`MSR3DFullStep.generate` is the reference's evaluation path (msr3d.py:445-524): prompt embeddings + scene tokens + one bos
embedding -> KV-cached greedy / beam search, nucleus sampling or beam sampling, `num_captions` results per prompt
(msr3d_amd/llm/generate.py) -> `output_tokens`.  `MSR3DFullStep.predict_answers` is
its closed-vocabulary path (msr3d.py:526-655): the same prompt, prefilled once, and the candidate answers scored as
short suffixes on that one cache (`rank_answers`) -> `answers_id`.  Parameter names: `visual_prompter.*`, `llm_proj.*` and
`llm_proj_img.*` as in the reference's MSR3D (a reference `pytorch_model.bin` loads them with no mapping); the language model
under `llm_model.*` (msr3d_amd/llm/checkpoint.py maps Hugging Face / peft keys onto it).

GPU only beyond the prompter: the language-model kernels have no CPU fallback."""
import torch
import torch.nn.functional as F

from .build import MODEL_REGISTRY
from .image_tokens import IMG_SP_TOKEN, MODES, project_scatter_images_, project_scatter_images_train_
from .scene_embeds import SCENE_SP_TOKEN, MSR3DHotPath, scatter_scene_embeds_, scatter_scene_embeds_train_


def build_targets(T_in, output_ids, output_mask):
    """msr3d.py:384-392: -100 everywhere except the answer's real tokens; the answer's first token (bos) is a
    condition, not a target.  No host sync (the reference's boolean-mask assignment is one)."""
    B = output_ids.shape[0]
    tail = torch.where(output_mask.bool(), output_ids, torch.full_like(output_ids, -100))
    tail[:, 0] = -100
    head = torch.full((B, T_in), -100, dtype=output_ids.dtype, device=output_ids.device)
    return torch.cat([head, tail], 1)


@MODEL_REGISTRY.register()
class MSR3DFullStep(MSR3DHotPath):
    """cfg: `prompter`, `llm_hidden_size` as MSR3DHotPath, plus `llm`: {num_layers, hidden_size, num_heads,
    intermediate_size, vocab_size, lora: {rank, alpha}, rms_eps, rope_theta, base: 'bf16' | 'fp8'}, optional `scene_sp_token` and `device`
    (the language model's weights -- 26 GB in both orientations for Vicuna-7B -- are created there directly).
    Optional `image_tokens`: {in_features: 1024, img_sp_token: 30861, image_mode: "interleaved" | "single"} adds the trainable
    `llm_proj_img` (nn.Linear(in_features, hidden)) and the image write for batches that carry `img_fts (B, N, in_features)` /
    `img_masks (B, N)`; without the block the model has no such parameter and nothing changes."""

    def __init__(self, cfg):
        super().__init__(cfg)
        from ..llm import LoRALlamaStack
        llm = cfg.llm
        if int(llm.hidden_size) != int(cfg.llm_hidden_size):
            raise ValueError("llm.hidden_size must equal llm_hidden_size (llm_proj's output width)")
        lora = llm.get("lora", {}) if hasattr(llm, "get") else {}
        dev = cfg.get("device", None) if hasattr(cfg, "get") else None
        img = cfg.get("image_tokens", None) if hasattr(cfg, "get") else None
        self.image_tokens = img is not None
        if self.image_tokens:
            # registered after llm_proj and before llm_model: reversed registration order stays the order backward produces
            # gradients (LoRA pairs, llm_proj_img, llm_proj, the prompter)
            self.img_sp_token = int(img.get("img_sp_token", IMG_SP_TOKEN))
            self.image_mode = str(img.get("image_mode", "interleaved"))
            if self.image_mode not in MODES:
                raise ValueError(f"image_tokens.image_mode must be one of {sorted(MODES)}")
            scene_tok = int(cfg.get("scene_sp_token", SCENE_SP_TOKEN))
            if not 0 <= self.img_sp_token < int(llm.vocab_size):
                raise ValueError("img_sp_token outside the vocabulary")
            if self.img_sp_token == scene_tok:
                raise ValueError("img_sp_token must differ from scene_sp_token")
            self.llm_proj_img = torch.nn.Linear(int(img.get("in_features", 1024)), int(llm.hidden_size))
        self.llm_model = LoRALlamaStack(int(llm.num_layers), int(llm.hidden_size), int(llm.num_heads),
                                        int(llm.intermediate_size), int(llm.vocab_size),
                                        r=int(lora.get("rank", 16)), lora_alpha=int(lora.get("alpha", 16)),
                                        rms_eps=float(llm.get("rms_eps", 1e-6)),
                                        rope_theta=float(llm.get("rope_theta", 10000.0)), device=dev,
                                        base=str(llm.get("base", "bf16")))
        self.register_buffer("embed_tokens", torch.zeros((int(llm.vocab_size), int(llm.hidden_size)),
                                                         dtype=torch.bfloat16, device=dev))
        self.scene_sp_token = int(cfg.get("scene_sp_token", SCENE_SP_TOKEN)) if hasattr(cfg, "get") else SCENE_SP_TOKEN
        if not 0 <= self.scene_sp_token < int(llm.vocab_size):
            raise ValueError("scene_sp_token outside the vocabulary")

    def get_opt_params(self):
        """Registration order = prompter, llm_proj, (llm_proj_img,) LoRA pairs layer 0..n-1: reversed by the gradient engine
        it is the order backward produces them (last decoder layer first, the prompter last)."""
        return [p for p in self.parameters() if p.requires_grad]

    def _write_images(self, emb, am, ids, data_dict, train):
        """msr3d.py:233-252, before the scene tokens: only when the block is configured; a batch without `img_fts` writes
        nothing.  train: through the autograd node, which is applied even then (n = 0, interleaved mode over one empty slot
        per row) so that llm_proj_img receives its -- zero -- gradient in every step."""
        if not self.image_tokens:
            return emb
        fts, msk, mode = data_dict.get("img_fts"), data_dict.get("img_masks"), self.image_mode
        if fts is None:
            if not (train and torch.is_grad_enabled()):
                return emb
            fts = emb.new_zeros((ids.shape[0], 1, self.llm_proj_img.in_features), dtype=torch.float32)
            msk, mode = torch.zeros((ids.shape[0], 1), dtype=torch.bool, device=ids.device), "interleaved"
        elif msk is None:
            raise KeyError("img_fts without img_masks")
        if train:
            return project_scatter_images_train_(emb, am, ids, fts, msk, self.llm_proj_img, self.img_sp_token, mode)
        project_scatter_images_(emb, am, ids, fts, msk, self.llm_proj_img, self.img_sp_token, mode)
        return emb

    def embed_inputs(self, data_dict, scene_embeds, scene_mask):
        """-> inputs_embeds (B, T, E) bf16 with the scene tokens written in, attention_mask (B, T) int64 with the
        object mask at the placeholder positions, targets (B, T)."""
        ids_in, am_in = data_dict["input_ids"], data_dict["attention_mask"]
        ids_out, am_out = data_dict["output_ids"], data_dict["output_mask"]
        ids = torch.cat([ids_in, ids_out], 1).contiguous()
        am = torch.cat([am_in, am_out], 1).to(torch.int64).contiguous()
        if ids.shape[1] % 64:
            raise ValueError("prompt + answer length must be a multiple of 64 tokens (left-pad the prompt)")
        emb = F.embedding(ids, self.embed_tokens)                         # (B, T, E) bf16, frozen table
        emb = self._write_images(emb, am, ids, data_dict, train=True)
        emb = scatter_scene_embeds_train_(emb, am, ids, scene_embeds, scene_mask, self.scene_sp_token)
        return emb, am, build_targets(ids_in.shape[1], ids_out, am_out)

    def forward(self, data_dict):
        """data_dict: the scene keys of MSR3DHotPath.forward + input_ids / attention_mask (B, T1) int64 (left-padded
        prompt with L scene placeholders per row) + output_ids / output_mask (B, T3) (right-padded answer + eos).
        -> data_dict with `loss` (B,) fp32 (and scene_embeds, obj_tokens, obj_masks from the hot path)."""
        if not data_dict["input_ids"].is_cuda:
            raise RuntimeError("MSR3DFullStep runs on the GPU only (the language-model kernels have no CPU fallback)")
        d = MSR3DHotPath.forward(self, data_dict)
        emb, am, targets = self.embed_inputs(d, d["scene_embeds"], d["obj_masks"])
        # (targets are -100 over the whole prompt by construction: the head and the loss run over the answer span only)
        d["loss"] = self.llm_model(emb, attention_mask=am, targets=targets, supervised_from=data_dict["input_ids"].shape[1])
        return d

    @torch.no_grad()
    def generate(self, data_dict, num_beams=5, max_length=256, min_length=1, repetition_penalty=3.0, length_penalty=1.0,
                 max_out_len=256, bos_id=1, eos_id=2, use_nucleus_sampling=False, top_p=0.9, temperature=1.0,
                 num_captions=1, seed=None, top_k=50, lora="separate", prompt_cache="rows", weights="bf16",
                 loop="host", poll=4, kv="bf16", step="split"):
        """The reference's MSR3D.generate: hot path -> prompt embeddings with the scene tokens written in and the object
        mask at their positions (prompt only, no answer) -> one bos embedding and a mask column of ones appended -> beam
        search (or sampling) over the key / value cache (`max_length` counts generated tokens) -> id 0 mapped to 2 ->
        padded with 2 to `max_out_len` -> data_dict['output_tokens'] (B x num_captions, max_out_len) int64, a prompt's
        captions in adjacent rows.
        use_nucleus_sampling = transformers' `do_sample`: with num_beams == 1 every caption is sampled token by token,
        with num_beams > 1 it is beam sampling; `top_p`, `temperature` and `top_k` act only then.  top_k: the reference
        never passes it, and the transformers it pins (4.28.1) then takes 50 whenever it samples -- so 50 is what the
        reference's sampled captions are drawn from and the default here; top_k=0 gives pure nucleus sampling.
        num_captions = `num_return_sequences`: the n best beams, or n samples per prompt.  seed: the draw's counter seed
        (None: 63 bits from torch's CPU generator, so torch.manual_seed makes a call reproducible).
        The prompt may have any length (the engine pads it to the attention kernel's multiple of 64 itself) and the batch
        any size (more than 64 rows = B x max(num_beams, num_captions) decode in groups of whole prompts).
        lora = "merged": decode on the language model's merged planes bf16(W + s B A) (LoRALlamaStack.merged_weights: one
        more copy of its projections in memory, rebuilt only after a weight was written; no low-rank launches).
        prompt_cache = "shared": the beams (or captions) of a prompt read ONE cached copy of the prompt's keys and values
        and carry only their generated tails (LoRALlamaStack.generate) -- the same tokens as the default "rows".
        weights = "e4m3": a model whose language model was built with base="fp8" decodes on its own e4m3 weights (the
        default "bf16" refuses such a model; LoRALlamaStack.generate).
        loop = "device": greedy and beam search with the token loop as graph replays, `done` read every `poll` tokens
        (LoRALlamaStack.generate; not with use_nucleus_sampling).
        kv = "e4m3": the key / value cache as e4m3 codes with a power-of-two scale per (slot, head): half the cache and
        half the attention's and the beam reorder's bytes; logits about 3 % rel-L2 from the default "bf16", so captions
        may differ (LoRALlamaStack.generate).
        step = "fused" (with lora="merged"): the decode step's norms, rotation and cache append inside its products, five
        launches a layer for eight -- the same tokens as the default "split" (LoRALlamaStack.generate)."""
        if not data_dict["input_ids"].is_cuda:
            raise RuntimeError("MSR3DFullStep runs on the GPU only (the language-model kernels have no CPU fallback)")
        if max_length > max_out_len:
            raise ValueError("max_length (generated tokens) must not exceed max_out_len")
        # the hot path with ordered reductions (hipops.set_deterministic: by default its split-K partial sums meet by float
        # atomics, 5e-6 apart from call to call -- enough to flip a bf16 scene token and, now and then, a beam): evaluation
        # output is the same tokens call after call; decoding itself has no atomics
        from .. import hipops
        was = hipops.set_deterministic(True)
        try:
            d = MSR3DHotPath.forward(self, data_dict)
        finally:
            hipops.set_deterministic(was)
        ids = data_dict["input_ids"].contiguous()
        am = data_dict["attention_mask"].to(torch.int64).contiguous().clone()
        emb = F.embedding(ids, self.embed_tokens).contiguous()
        self._write_images(emb, am, ids, data_dict, train=False)
        scatter_scene_embeds_(emb, am, ids, d["scene_embeds"].detach(), d["obj_masks"], self.scene_sp_token)
        out = self.llm_model.generate(emb, am, self.embed_tokens, bos_id=bos_id, eos_id=eos_id, pad_id=eos_id,
                                      num_beams=num_beams, max_length=max_length, min_length=min_length,
                                      repetition_penalty=repetition_penalty, length_penalty=length_penalty,
                                      do_sample=bool(use_nucleus_sampling), top_p=top_p, top_k=top_k,
                                      temperature=temperature, num_return_sequences=num_captions, seed=seed, lora=lora,
                                      prompt_cache=prompt_cache, weights=weights, loop=loop, poll=poll, kv=kv,
                                      step=step)
        out = torch.where(out == 0, torch.full_like(out, 2), out)
        pad = torch.full((out.shape[0], max_out_len - out.shape[1]), 2, dtype=out.dtype, device=out.device)
        d["output_tokens"] = torch.cat([out, pad], 1)
        return d

    @torch.no_grad()
    def predict_answers(self, data_dict, answer_ids, answer_mask, num_ans_candidates=128, bos_id=1, answer_list=None,
                        lora="separate", weights="bf16"):
        """The reference's MSR3D.predict_answers: hot path -> prompt embeddings with the scene tokens written in and the
        object mask at their positions -> one bos embedding and a mask column of ones appended -> the `num_ans_candidates`
        answers whose first token is most probable -> the one with the smallest mean token loss ->
        data_dict['answers_id'] (B,) int64 on the device (indices into the answer list), plus 'answers_topk_ids' (B, C),
        'answers_loss' (B, C) fp32 and, with `answer_list` (the strings), 'answers'.  answer_ids / answer_mask (A, S) int64:
        the tokenised answer list, bos first, right-padded (tokenising stays outside, like all tokenising here).
        lora: "separate" or "merged", weights: "bf16" or "e4m3", as in `generate`."""
        if not data_dict["input_ids"].is_cuda:
            raise RuntimeError("MSR3DFullStep runs on the GPU only (the language-model kernels have no CPU fallback)")
        if answer_list is not None and len(answer_list) != answer_ids.shape[0]:
            raise ValueError("answer_list and answer_ids disagree on the number of answers")
        # (deterministic hot path: see generate -- a flipped bf16 scene token could flip a close ranking)
        from .. import hipops
        was = hipops.set_deterministic(True)
        try:
            d = MSR3DHotPath.forward(self, data_dict)
        finally:
            hipops.set_deterministic(was)
        ids = data_dict["input_ids"].contiguous()
        am = data_dict["attention_mask"].to(torch.int64).contiguous().clone()
        emb = F.embedding(ids, self.embed_tokens).contiguous()
        self._write_images(emb, am, ids, data_dict, train=False)
        scatter_scene_embeds_(emb, am, ids, d["scene_embeds"].detach(), d["obj_masks"], self.scene_sp_token)
        out = self.llm_model.predict_answers(emb, am, self.embed_tokens, answer_ids, answer_mask,
                                             num_ans_candidates=num_ans_candidates, bos_id=bos_id, lora=lora,
                                             weights=weights)
        d["answers_id"] = out["answers_id"]
        d["answers_topk_ids"], d["answers_loss"] = out["topk_ids"], out["loss"]
        if answer_list is not None:
            d["answers"] = [answer_list[i] for i in out["answers_id"].tolist()]
        return d
