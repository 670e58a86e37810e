"""CPU: the image-token hand-off (msr3d_amd/model/image_tokens.py) -- the sync-free torch mirror against the LITERAL procedure
of the reference's MSR3D.build_embeds, written out here (torch.where(input_ids == tok) + boolean-mask compaction + indexed
assignment), and the opt-in `image_tokens` block of MSR3DFullStep (parameter names, registration order, validation)."""
import numpy as np
import pytest
import torch

TOK = 77


def literal(emb, am, ids, tokens, masks, mode):
    """The reference's statements, host syncs and all; on a count mismatch the first min(placeholders, sources) pairs."""
    emb, am = emb.clone(), am.clone()
    idx = torch.where(ids == TOK)                                     # row-major
    if mode == "interleaved":
        if int(masks.sum()) == 0:                                     # `if img_mask.sum(1).sum(0) > 0`
            return emb, am
        src = tokens[masks.bool()]                                    # boolean-mask compaction, row-major
    else:
        src = tokens.reshape(-1, tokens.shape[-1])
    n = min(idx[0].numel(), src.shape[0])
    idx = (idx[0][:n], idx[1][:n])
    emb[idx] = src[:n].to(emb.dtype)
    if mode == "single":
        am[idx] = masks.reshape(-1)[:n].to(am.dtype)
    return emb, am


def make(seed, B, T, N, E, counts, placeholders=None, dtype=torch.bfloat16):
    """counts[b] masked slots (the first ones) and placeholders[b] (default = counts[b]) placeholder tokens in row b."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(100, 1000, (B, T))
    placeholders = counts if placeholders is None else placeholders
    for b in range(B):
        ids[b, np.sort(rng.choice(T, placeholders[b], replace=False))] = TOK
    masks = np.zeros((B, N), bool)
    for b in range(B):
        masks[b, :counts[b]] = True
    emb = torch.from_numpy(rng.standard_normal((B, T, E)).astype(np.float32)).to(dtype)
    am = torch.from_numpy(rng.integers(0, 2, (B, T)).astype(np.int64))
    tokens = torch.from_numpy(rng.standard_normal((B, N, E)).astype(np.float32))
    return emb, am, torch.from_numpy(ids), tokens, torch.from_numpy(masks)


CASES = {
    "mixed_rows": dict(B=4, T=40, N=6, counts=[0, 6, 3, 1]),                      # a row with none, a row with all N
    "no_image": dict(B=3, T=24, N=4, counts=[0, 0, 0]),
    "every_slot": dict(B=2, T=16, N=5, counts=[5, 5]),
    "surplus_placeholders": dict(B=3, T=30, N=4, counts=[1, 2, 0], placeholders=[3, 2, 2]),
    "surplus_images": dict(B=3, T=30, N=4, counts=[4, 3, 2], placeholders=[1, 0, 3]),
    "no_image_but_placeholders": dict(B=2, T=12, N=3, counts=[0, 0], placeholders=[2, 1]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_interleaved_mirror_equals_the_literal_procedure(name):
    from msr3d_amd.model.image_tokens import scatter_image_tokens
    c = CASES[name]
    emb, am, ids, tokens, masks = make(3, c["B"], c["T"], c["N"], 8, c["counts"], c.get("placeholders"))
    want_e, want_m = literal(emb, am, ids, tokens, masks, "interleaved")
    keep = emb.clone()
    got_e, got_m = scatter_image_tokens(emb, am, ids, tokens, masks, img_sp_token=TOK, mode="interleaved")
    assert torch.equal(got_e, want_e) and torch.equal(got_m, want_m)
    assert torch.equal(got_m, am)                                     # the mask is not touched in this mode
    assert torch.equal(emb, keep)                                     # new tensors, the inputs stay
    placeholders = c.get("placeholders", c["counts"])
    n = min(sum(placeholders), sum(c["counts"]))
    assert int((got_e != emb).any(-1).sum()) == n                     # exactly the first min pairs were written


@pytest.mark.parametrize("placeholders,slots", [([1, 1, 1, 1, 1], 5), ([1, 1, 0, 1, 0], 5), ([2, 2, 1, 1, 1], 5)])
def test_single_mirror_equals_the_literal_procedure(placeholders, slots):
    """"single": every slot is a source, masked or not; the mask entry of the slot lands in attention_mask.  Fewer and more
    placeholders than slots: the first min pairs."""
    from msr3d_amd.model.image_tokens import scatter_image_tokens
    B = slots
    emb, am, ids, tokens, masks = make(5, B, 20, 1, 8, [1, 0, 1, 0, 1], placeholders)
    am[ids == TOK] = 7                                                # (a written entry differs from what was there)
    want_e, want_m = literal(emb, am, ids, tokens, masks, "single")
    got_e, got_m = scatter_image_tokens(emb, am, ids, tokens, masks, img_sp_token=TOK, mode="single")
    assert torch.equal(got_e, want_e) and torch.equal(got_m, want_m)
    n = min(sum(placeholders), B)
    hit = torch.where(ids == TOK)
    assert torch.equal(got_m[hit][:n], masks.reshape(-1)[:n].to(torch.int64))
    rest = torch.ones_like(am, dtype=torch.bool)
    rest[(hit[0][:n], hit[1][:n])] = False
    assert torch.equal(got_m[rest], am[rest]) and torch.equal(got_e[rest], emb[rest])


def test_synth_images_places_exactly_the_requested_placeholders():
    from msr3d_amd.synth import synth_images, synth_text
    text = synth_text(11, 4, L=6, T_in=48, T_out=16, vocab=300, scene_token=299)
    counts = [0, 4, 2, 1]
    img = synth_images(12, text, N=4, C=32, img_token=250, counts=counts, scene_token=299)
    ids, old = img["input_ids"], text["input_ids"]
    assert (ids == 250).sum(1).tolist() == counts
    assert img["img_masks"].sum(1).tolist() == counts and img["img_masks"][1].all()
    changed = ids != old
    assert not (changed & ((old == 299) | (old == 1) | (text["attention_mask"] == 0))).any()
    assert torch.equal((ids == 299), (old == 299))
    assert img["img_fts"].shape == (4, 4, 32) and img["img_fts"].dtype == torch.float32
    one = synth_images(12, text, N=1, C=32, img_token=250, counts=[1, 0, 1, 0], mode="single", scene_token=299)
    assert (one["input_ids"] == 250).sum(1).tolist() == [1, 1, 1, 1] and one["img_masks"][:, 0].tolist() == [True, False, True, False]


def _cfg(image_tokens=None):
    from msr3d_amd.config import AttrDict, default_prompter_cfg
    cfg = {"prompter": default_prompter_cfg(dropout=0.0), "llm_hidden_size": 128,
           "llm": {"num_layers": 1, "hidden_size": 128, "num_heads": 2, "intermediate_size": 256, "vocab_size": 320,
                   "lora": {"rank": 16, "alpha": 16}},
           "scene_sp_token": 300, "model": {"name": "MSR3DFullStep"}}
    if image_tokens is not None:
        cfg["image_tokens"] = image_tokens
    return AttrDict(cfg)


def test_full_step_registers_llm_proj_img_only_when_asked():
    import msr3d_amd.model  # noqa: F401
    import msr3d_amd.modules  # noqa: F401
    from msr3d_amd.model import build_model
    plain = build_model(_cfg())
    keys = list(plain.state_dict())
    assert not any("llm_proj_img" in k for k in keys)
    assert not hasattr(plain, "llm_proj_img")
    assert all(k.startswith(("visual_prompter.", "llm_proj.", "llm_model.")) or k == "embed_tokens" for k in keys)
    with_img = build_model(_cfg({"in_features": 64, "img_sp_token": 301, "image_mode": "interleaved"}))
    keys_img = list(with_img.state_dict())
    assert set(keys_img) - set(keys) == {"llm_proj_img.weight", "llm_proj_img.bias"} and set(keys) <= set(keys_img)
    assert [k for k in keys_img if "llm_proj_img" not in k] == keys                   # nothing else moved
    assert tuple(with_img.llm_proj_img.weight.shape) == (128, 64) and with_img.llm_proj_img.weight.dtype == torch.float32
    # registered between llm_proj.* and llm_model.*: reversed, the order backward produces the gradients
    names = [n for n, _ in with_img.named_parameters()]
    i = names.index("llm_proj_img.weight")
    assert names[i - 2:i + 2] == ["llm_proj.weight", "llm_proj.bias", "llm_proj_img.weight", "llm_proj_img.bias"]
    assert names[i + 2].startswith("llm_model.") and all(n.startswith("llm_model.") for n in names[i + 2:])
    assert any(p is with_img.llm_proj_img.weight for p in with_img.get_opt_params())
    assert [n for n, _ in plain.named_parameters()] == [n for n in names if "llm_proj_img" not in n]


@pytest.mark.parametrize("tok,why", [(320, "vocabulary"), (-1, "vocabulary"), (300, "scene_sp_token")])
def test_full_step_rejects_a_bad_img_sp_token(tok, why):
    import msr3d_amd.model  # noqa: F401
    import msr3d_amd.modules  # noqa: F401
    from msr3d_amd.model import build_model
    with pytest.raises(ValueError, match=why):
        build_model(_cfg({"in_features": 64, "img_sp_token": tok}))
    with pytest.raises(ValueError, match="image_mode"):
        build_model(_cfg({"in_features": 64, "img_sp_token": 301, "image_mode": "tiled"}))
