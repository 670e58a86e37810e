"""GPU: image tokens inside the full step (MSR3DFullStep with the `image_tokens` block; msr3d_amd/model/image_tokens.py) on
the small model of tests/test_full_step_gpu.py (its build_model / make_batch, the sizes of full_step_seed0.npz), image
placeholder id 1001 inside that vocabulary, C = 64 features, N = 4 slots.

Bounds as in tests/test_image_tokens_gpu.py (u = 2^-24): an image row within 4 (C + 2) u S + 2^-8 |y64| of the float64
projection; llm_proj_img's gradients within 4 (n + 2) u sum_k |G_k f_k| of the float64 product of the captured d inputs_embeds.
The captured-graph comparison uses exactly the bounds of test_full_step_captured_graph_replays_the_eager_steps."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
IMG_TOK, C_IMG, N_IMG = 1001, 64, 4


def fixture_file():
    return dict(np.load(os.path.join(GOLD, "full_step_seed0.npz"), allow_pickle=False))


def build(g, images=True, dropout=0.0):
    """tests.test_full_step_gpu.build_model, with the `image_tokens` block added to the configuration it builds."""
    import msr3d_amd.model as mm
    from tests.test_full_step_gpu import build_model
    orig = mm.build_model

    def with_block(cfg):
        if images:
            cfg.image_tokens = {"in_features": C_IMG, "img_sp_token": IMG_TOK, "image_mode": "interleaved"}
        return orig(cfg)
    mm.build_model = with_block
    try:
        model, c = build_model(g, dropout=dropout)
    finally:
        mm.build_model = orig
    if images:
        gen = torch.Generator().manual_seed(int(g["seed"]) + 200)
        with torch.no_grad():
            model.llm_proj_img.weight.copy_(torch.randn(c["hidden"], C_IMG, generator=gen) / C_IMG ** 0.5)
            model.llm_proj_img.bias.copy_(0.1 * torch.randn(c["hidden"], generator=gen))
    return model, c


def batch_of(c, i, counts, B=None, keys=True):
    from msr3d_amd.synth import synth_batch, synth_images, synth_text
    B = c["B"] if B is None else B
    batch = synth_batch(8000 + i, B, O=c["O"], P=c["P"], n_valid=[c["O"] - c["n_pad"]] * B, device="cuda")
    batch.update(synth_text(8100 + i, B, L=c["O"], T_in=c["T_in"], T_out=c["T_out"], vocab=c["vocab"],
                            scene_token=c["scene_token"], device="cuda"))
    if counts is not None:
        img = synth_images(8200 + i, batch, N_IMG, C_IMG, IMG_TOK, counts=counts, scene_token=c["scene_token"])
        if not keys:
            img = {"input_ids": img["input_ids"]}
        batch.update(img)
    return batch


@pytest.fixture(scope="module")
def models():
    g = fixture_file()
    model, c = build(g)
    plain, _ = build(g, images=False)
    return model, plain, c


def projection64(model, batch):
    """float64: (flat placeholder rows, y64, S, the real images' features) by the literal procedure."""
    ids = torch.cat([batch["input_ids"], batch["output_ids"]], 1).cpu() if "output_ids" in batch else batch["input_ids"].cpu()
    dest = torch.nonzero(ids.reshape(-1) == IMG_TOK).reshape(-1)
    f = batch["img_fts"].cpu()[batch["img_masks"].cpu()].double()
    W, b = model.llm_proj_img.weight.detach().cpu().double(), model.llm_proj_img.bias.detach().cpu().double()
    return dest, f @ W.T + b, f.abs() @ W.abs().T + b.abs(), f


def test_embed_inputs_writes_image_rows_and_trains_llm_proj_img(models):
    from msr3d_amd.model.scene_embeds import MSR3DHotPath
    model, _, c = models
    model.train()
    model.zero_grad(set_to_none=True)
    batch = batch_of(c, 0, [4, 1])
    no_keys = {k: v for k, v in batch.items() if k not in ("img_fts", "img_masks")}
    d = MSR3DHotPath.forward(model, dict(batch))
    with torch.no_grad():
        emb0, am0, _ = model.embed_inputs(no_keys, d["scene_embeds"].detach(), d["obj_masks"])
    emb, am, targets = model.embed_inputs(batch, d["scene_embeds"], d["obj_masks"])
    seen = {}
    emb.register_hook(lambda gr: seen.__setitem__("g", gr.detach().clone()))
    E = emb.shape[-1]
    dest, y64, S, f64 = projection64(model, batch)
    n = dest.numel()
    assert n == 5
    got = emb.detach().reshape(-1, E).cpu()[dest].double()
    bound = 4 * (C_IMG + 2) * U * S + 2.0 ** -8 * y64.abs()
    print("image rows: max err / bound", float(((got - y64).abs() / bound).max()))
    assert bool(((got - y64).abs() <= bound).all())
    rest = torch.ones(emb.shape[0] * emb.shape[1], dtype=torch.bool)
    rest[dest] = False
    assert torch.equal(emb.detach().reshape(-1, E).cpu()[rest], emb0.reshape(-1, E).cpu()[rest])     # scene rows included
    scene_rows = torch.cat([batch["input_ids"], batch["output_ids"]], 1).reshape(-1) == c["scene_token"]
    assert int(scene_rows.sum()) == c["B"] * c["O"] and not bool(scene_rows.cpu()[dest].any())
    assert torch.equal(am, am0)
    loss = model.llm_model(emb, attention_mask=am, targets=targets, supervised_from=batch["input_ids"].shape[1]).mean()
    loss.backward()
    torch.cuda.synchronize()
    g64 = seen["g"].reshape(-1, E).cpu()[dest].double()
    assert float(g64.abs().max()) > 0.0
    dW, db = model.llm_proj_img.weight.grad.cpu().double(), model.llm_proj_img.bias.grad.cpu().double()
    bW, bb = 4 * (n + 2) * U * (g64.abs().T @ f64.abs()), 4 * (n + 2) * U * g64.abs().sum(0)
    print("d llm_proj_img: max err / bound", float(((dW - g64.T @ f64).abs() / bW).max()), float(((db - g64.sum(0)).abs() / bb).max()))
    assert bool(((dW - g64.T @ f64).abs() <= bW).all()) and bool(((db - g64.sum(0)).abs() <= bb).all())
    lora = model.llm_model.layers[0].self_attn["q_proj"].lora_B.weight.grad
    for gr in (model.visual_prompter.spatial_encoder[0].linear1.weight.grad, model.llm_proj.weight.grad, lora):
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0.0
    model.zero_grad(set_to_none=True)


def test_probe_on_an_image_free_batch_keeps_llm_proj_img_trainable():
    from msr3d_amd.full_step import FullTrainStep
    g = fixture_file()
    model, c = build(g)
    ts = FullTrainStep(model, lr=2e-3, weight_decay=0.0, max_grad_norm=1.0)
    w, b = model.llm_proj_img.weight, model.llm_proj_img.bias
    order = [id(p) for p in ts.dp.order]
    # reversed registration order: LoRA pairs, then llm_proj_img, then llm_proj, then the prompter
    assert order.index(id(b)) + 1 == order.index(id(w)) and order.index(id(w)) + 1 == order.index(id(model.llm_proj.bias))
    frozen = [model.llm_model.lm_head.weight.clone(), model.embed_tokens.clone()] + \
             [p.detach().clone() for p in model.visual_prompter.obj_encoder.parameters()]
    w0 = w.detach().clone()
    ts(batch_of(c, 0, None))                                            # the probe (and one step) on a batch without image keys
    unused = {id(p) for p in ts.unused_parameters}
    assert id(w) not in unused and id(b) not in unused
    assert id(model.visual_prompter.anchor_feat) in unused            # (the probe still finds what IS unused)
    off, k = ts.dp.offset[id(w)], w.numel()
    assert float(ts.opt.exp_avg[off:off + k].abs().max()) == 0.0 and torch.equal(w.detach(), w0)   # zero gradient so far
    ts(batch_of(c, 1, [3, 1]))
    torch.cuda.synchronize()
    assert float(ts.opt.exp_avg[off:off + k].abs().max()) > 0.0 and not torch.equal(w.detach(), w0)
    now = [model.llm_model.lm_head.weight, model.embed_tokens] + list(model.visual_prompter.obj_encoder.parameters())
    assert all(torch.equal(a, b_) for a, b_ in zip(frozen, now))


def test_captured_graph_with_rotating_image_counts_replays_the_eager_steps():
    from msr3d_amd.full_step import FullTrainStep
    g = fixture_file()
    counts = [[0, 0, 0, 0], [1, 0, 3, 0], [4, 4, 4, 4]]
    outs = []
    for use_graph in (False, True):
        model, c = build(g)
        ts = FullTrainStep(model, lr=1e-3, weight_decay=0.0, max_grad_norm=1.0, use_graph=use_graph)
        losses = [float(ts(batch_of(c, i, counts[i % 3], B=4))) for i in range(5)]
        torch.cuda.synchronize()
        assert (ts.graph is not None) == use_graph
        w = model.llm_proj_img.weight
        off = ts.dp.offset[id(w)]
        outs.append((losses, ts.opt.flat_p.detach().clone(), ts.opt.exp_avg[off:off + w.numel()].clone()))
    (l0, p0, m0), (l1, p1, m1) = outs
    assert np.allclose(l0, l1, rtol=2e-3), (l0, l1)
    assert float((p0 - p1).abs().max()) < 5e-3 and float(((p0 - p1).abs() > 1e-4).float().mean()) < 0.02
    assert float(m0.abs().max()) > 0.0 and float(m1.abs().max()) > 0.0          # the replayed steps trained llm_proj_img too


def kernel_rows(model, fts):
    """Every slot's token in bf16 exactly as the kernel writes it: each slot as its own one-token sequence."""
    from msr3d_amd.model.image_tokens import project_scatter_images_
    B, N, C = fts.shape
    emb = torch.zeros(B * N, 1, model.llm_proj_img.out_features, dtype=torch.bfloat16, device=fts.device)
    ids = torch.full((B * N, 1), IMG_TOK, dtype=torch.int64, device=fts.device)
    with torch.no_grad():
        project_scatter_images_(emb, None, ids, fts.reshape(B * N, 1, C), torch.ones(B * N, 1, dtype=torch.bool, device=fts.device),
                                model.llm_proj_img, IMG_TOK, "single")
    return emb.reshape(B, N, -1)


class prewritten:
    """The image rows written into the embedding path by the TEST (the torch mirror, the kernel's own bf16 rows), in front of
    the scene scatter of generate / predict_answers."""

    def __init__(self, model, fts, masks):
        self.rows, self.masks = kernel_rows(model, fts), masks

    def __enter__(self):
        import msr3d_amd.model.msr3d_full as mf
        from msr3d_amd.model.image_tokens import scatter_image_tokens
        self.mf, self.orig = mf, mf.scatter_scene_embeds_

        def scatter(emb, am, ids, *a, **kw):
            emb.copy_(scatter_image_tokens(emb, am, ids, self.rows, self.masks, IMG_TOK, "interleaved")[0])
            return self.orig(emb, am, ids, *a, **kw)
        mf.scatter_scene_embeds_ = scatter

    def __exit__(self, *exc):
        self.mf.scatter_scene_embeds_ = self.orig
        return False


def other_features(batch):
    gen = torch.Generator().manual_seed(99)
    return 4.0 * torch.randn(batch["img_fts"].shape, generator=gen).to(batch["img_fts"].device)


def test_generate_sees_the_images(models):
    model, plain, c = models
    model.eval()
    plain.eval()
    kw = dict(num_beams=1, max_length=8, max_out_len=8, min_length=1)                # greedy
    batch = batch_of(c, 2, [4, 2])
    no_keys = {k: v for k, v in batch.items() if k not in ("img_fts", "img_masks")}
    tok = model.generate(dict(batch), **kw)["output_tokens"]
    with prewritten(model, batch["img_fts"], batch["img_masks"]):
        want = model.generate(dict(no_keys), **kw)["output_tokens"]
    assert torch.equal(tok, want), (tok, want)
    other = model.generate(dict(batch, img_fts=other_features(batch)), **kw)["output_tokens"]
    print("generate:", tok.tolist(), "other images:", other.tolist())
    assert not torch.equal(tok, other)
    # the block configured, no image keys: the model without the block
    text = batch_of(c, 2, None)
    assert torch.equal(model.generate(dict(text), **kw)["output_tokens"], plain.generate(dict(text), **kw)["output_tokens"])


def test_predict_answers_sees_the_images(models):
    from tests.predict_helpers import answer_set
    model, plain, c = models
    model.eval()
    plain.eval()
    ids, am = answer_set(5, A=24, S=6, vocab=c["vocab"])
    ids, am = ids.cuda(), am.cuda()
    batch = batch_of(c, 3, [2, 4])
    no_keys = {k: v for k, v in batch.items() if k not in ("img_fts", "img_masks")}
    keys = ("answers_id", "answers_topk_ids", "answers_loss")
    got = model.predict_answers(dict(batch), ids, am, num_ans_candidates=8)
    with prewritten(model, batch["img_fts"], batch["img_masks"]):
        want = model.predict_answers(dict(no_keys), ids, am, num_ans_candidates=8)
    for k in keys:
        assert torch.equal(got[k], want[k]), k
    other = model.predict_answers(dict(batch, img_fts=other_features(batch)), ids, am, num_ans_candidates=8)
    print("predict_answers:", got["answers_id"].tolist(), got["answers_topk_ids"].tolist(), "other images:",
          other["answers_id"].tolist(), other["answers_topk_ids"].tolist())
    assert not (torch.equal(got["answers_topk_ids"], other["answers_topk_ids"]) and torch.equal(got["answers_loss"], other["answers_loss"]))
    text = batch_of(c, 3, None)
    a, b = model.predict_answers(dict(text), ids, am, num_ans_candidates=8), plain.predict_answers(dict(text), ids, am, num_ans_candidates=8)
    for k in keys:
        assert torch.equal(a[k], b[k]), k
