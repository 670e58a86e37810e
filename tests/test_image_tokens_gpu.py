"""GPU: the image-token kernels (msr3d_amd/csrc/image_tokens.hip through msr3d_amd/model/image_tokens.py) against float64.

Shapes: the smallest that cross every boundary of the kernels.  Main case B = 3, T = 300 (a row crosses the 256-position
scan), N = 40 with per-row counts [0, 40, 27] (n = 67 crosses a 64-row band and a 16-row gradient slab; one row without an
image), C = 96 (three K slabs, no power of two), E = 256 (two column slabs, four gradient row tiles); row 1 has placeholders
at positions 0, 255, 256, T - 1 and a run of adjacent ones.

Bounds (derived, not measured; u = 2^-24):
  forward   an fp32 dot product of C terms plus bias errs, in any order, by at most (C + 1) u S to first order,
            S = sum_i |W_ei f_i| + |b_e| in float64; four times that: |y - y64| <= 4 (C + 2) u S for fp32 output, plus
            2^-8 |y64| (one rounding to nearest) for bf16 output.
  backward  G in bf16: |dW - dW64| <= 4 (n + 2) u sum_k |G_ke f_kc|, |db - db64| <= 4 (n + 2) u sum_k |G_ke|.
            accumulate = 1 onto an N(0, 1) prefill: the same bound on the difference (the add's own rounding, u |p + a| with
            |p + a| of order 10, is three orders below the bound at n = 67)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TOK = 30861
DEV = "cuda"


def layout(B, T, rows):
    ids = np.random.default_rng(1).integers(3, 30000, (B, T))
    for b, pos in enumerate(rows):
        ids[b, pos] = TOK
    return torch.from_numpy(ids)


def problem(seed, B, T, N, C, E, counts, rows, dtype=torch.bfloat16, masks=None):
    g = torch.Generator().manual_seed(seed)
    ids = layout(B, T, rows)
    if masks is None:
        masks = torch.zeros(B, N, dtype=torch.bool)
        for b, c in enumerate(counts):
            masks[b, :c] = True
    p = {"ids": ids, "masks": masks, "fts": torch.randn(B, N, C, generator=g),
         "W": torch.randn(E, C, generator=g) / C ** 0.5, "b": torch.randn(E, generator=g),
         "emb": torch.randn(B, T, E, generator=g).to(dtype), "am": torch.randint(0, 2, (B, T), generator=g)}
    return p


def reference(p, mode):
    """float64, by the literal procedure: (dest rows, src slots, y64 (n, E), S (n, E))."""
    dest = torch.nonzero(p["ids"].reshape(-1) == TOK).reshape(-1)
    src = torch.nonzero(p["masks"].reshape(-1)).reshape(-1) if mode == "interleaved" else torch.arange(p["masks"].numel())
    n = min(dest.numel(), src.numel())
    dest, src = dest[:n], src[:n]
    f = p["fts"].reshape(-1, p["fts"].shape[-1]).double()[src]
    y = f @ p["W"].double().T + p["b"].double()
    S = f.abs() @ p["W"].double().abs().T + p["b"].double().abs()
    return dest, src, y, S


def run_forward(p, mode, dtype=None):
    from msr3d_amd.model import image_tokens as it
    emb = p["emb"].to(DEV) if dtype is None else p["emb"].float().to(dtype).to(DEV)
    am = p["am"].to(DEV)
    lin = torch.nn.Linear(p["W"].shape[1], p["W"].shape[0]).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(p["W"])
        lin.bias.copy_(p["b"])
        before, am0 = emb.clone(), am.clone()
        dest, src, cnt, fts = it._launch(emb, am, p["ids"].to(DEV), p["fts"].to(DEV), p["masks"].to(DEV), lin.weight,
                                         lin.bias, TOK, mode)
    torch.cuda.synchronize()
    return dict(emb=emb.cpu(), am=am.cpu(), before=before.cpu(), am0=am0.cpu(), dest=dest, src=src, cnt=cnt, fts=fts)


def check_forward(p, out, mode, bf16):
    dest, src, y, S = reference(p, mode)
    n, C, E = dest.numel(), p["W"].shape[1], p["W"].shape[0]
    assert out["cnt"].tolist() == [int((p["ids"] == TOK).sum()),
                                   int(p["masks"].sum()) if mode == "interleaved" else p["masks"].numel()]
    assert torch.equal(out["dest"][:n].cpu().long(), dest) and torch.equal(out["src"][:n].cpu().long(), src)
    got = out["emb"].reshape(-1, E)[dest].double()
    bound = 4 * (C + 2) * U * S + (2.0 ** -8 * y.abs() if bf16 else 0.0)
    err = (got - y).abs()
    print(f"forward n={n} max err / bound = {float((err / bound).max()) if n else 0.0:.3e}")
    assert bool((err <= bound).all())
    rest = torch.ones(out["emb"].shape[0] * out["emb"].shape[1], dtype=torch.bool)
    rest[dest] = False
    assert torch.equal(out["emb"].reshape(-1, E)[rest], out["before"].reshape(-1, E)[rest])      # bit-identical elsewhere
    if mode == "interleaved":
        assert torch.equal(out["am"], out["am0"])
    else:
        assert torch.equal(out["am"].reshape(-1)[dest], p["masks"].reshape(-1)[src].to(torch.int64))
        assert torch.equal(out["am"].reshape(-1)[rest], out["am0"].reshape(-1)[rest])
    return dest, src


ROW1 = [0, 255, 256, 299] + list(range(100, 136))                      # 40 placeholders: the edges, the scan seam, a run
ROW2 = sorted(np.random.default_rng(2).choice(300, 27, replace=False).tolist())
MAIN = dict(B=3, T=300, N=40, C=96, E=256, counts=[0, 40, 27], rows=[[], ROW1, ROW2])


@pytest.fixture(scope="module")
def main_case():
    p = problem(0, **MAIN)
    return p, run_forward(p, "interleaved")


def test_forward_main_case_bf16(main_case):
    p, out = main_case
    dest, _ = check_forward(p, out, "interleaved", bf16=True)
    assert dest.numel() == 67


def test_forward_main_case_fp32_output():
    p = problem(0, **MAIN)
    check_forward(p, run_forward(p, "interleaved", torch.float32), "interleaved", bf16=False)


@pytest.mark.parametrize("counts,rows", [([0, 0], [[], []]), ([0, 1], [[], [17]])])
def test_forward_no_image_and_one_image(counts, rows):
    p = problem(3, B=2, T=64, N=3, C=32, E=128, counts=counts, rows=rows)
    out = run_forward(p, "interleaved")
    check_forward(p, out, "interleaved", bf16=True)
    if sum(counts) == 0:
        assert torch.equal(out["emb"], out["before"])


def test_forward_single_mode_writes_the_slot_mask():
    masks = torch.tensor([[True], [False], [True], [False], [True]])
    p = problem(4, B=5, T=64, N=1, C=32, E=128, counts=None, rows=[[5], [63], [0], [31], [32]], masks=masks)
    p["am"][p["ids"] == TOK] = 7                                       # (a written entry differs from what was there)
    out = run_forward(p, "single")
    dest, _ = check_forward(p, out, "single", bf16=True)
    assert dest.numel() == 5


@pytest.mark.parametrize("counts,rows,n", [([1, 2], [[3, 70], [1, 2, 299]], 3),      # 5 placeholders, 3 images
                                           ([4, 3], [[9], [250, 257]], 3)])           # 3 placeholders, 7 images
def test_forward_count_mismatch_writes_the_first_pairs(counts, rows, n):
    p = problem(5, B=2, T=300, N=4, C=32, E=128, counts=counts, rows=rows)
    out = run_forward(p, "interleaved")
    dest, _ = check_forward(p, out, "interleaved", bf16=True)        # (surplus placeholders: bit-identical to before)
    assert dest.numel() == n and out["cnt"].tolist() == [sum(len(r) for r in rows), sum(counts)]
    from msr3d_amd.model import image_tokens as it
    lin = torch.nn.Linear(32, 128).to(DEV)
    with torch.no_grad(), pytest.raises(RuntimeError, match="placeholders"):
        it.project_scatter_images_(p["emb"].to(DEV), None, p["ids"].to(DEV), p["fts"].to(DEV), p["masks"].to(DEV), lin, TOK,
                                   validate=True)


def grads(p, out, G, accumulate, prefill=None, clear=True):
    from msr3d_amd.model import image_tokens as it
    E, C = p["W"].shape
    g = G.clone().to(DEV)
    if prefill is None:
        dW, db = torch.full((E, C), float("nan"), device=DEV), torch.full((E,), float("nan"), device=DEV)
    else:
        dW, db = prefill[0].clone().to(DEV), prefill[1].clone().to(DEV)
    it.image_project_grad(g, out["dest"], out["src"], out["cnt"], out["fts"], dW, db, accumulate=accumulate, clear_rows=clear)
    torch.cuda.synchronize()
    return dW.cpu(), db.cpu(), g.cpu()


def check_backward(p, out, G, dtype_name=""):
    dest, src, _, _ = reference(p, "interleaved")
    n = dest.numel()
    E, C = p["W"].shape
    g64 = G.reshape(-1, E)[dest].double()
    f64 = p["fts"].reshape(-1, C)[src].double()
    dW64, db64 = g64.T @ f64, g64.sum(0)
    bW, bb = 4 * (n + 2) * U * (g64.abs().T @ f64.abs()), 4 * (n + 2) * U * g64.abs().sum(0)
    dW, db, g_after = grads(p, out, G, accumulate=False)
    print(f"backward{dtype_name} n={n} dW err/bound {float(((dW.double() - dW64).abs() / bW.clamp_min(1e-300)).max()):.3e} "
          f"db err/bound {float(((db.double() - db64).abs() / bb.clamp_min(1e-300)).max()):.3e}")
    assert bool(((dW.double() - dW64).abs() <= bW).all()) and bool(((db.double() - db64).abs() <= bb).all())
    # the placeholder rows are cleared, every other row is untouched
    rest = torch.ones(G.shape[0] * G.shape[1], dtype=torch.bool)
    rest[dest] = False
    assert float(g_after.reshape(-1, E)[dest].float().abs().sum()) == 0.0
    assert torch.equal(g_after.reshape(-1, E)[rest], G.reshape(-1, E)[rest])
    return dW64, db64, bW, bb, (dW, db)


def test_backward_main_case_store_accumulate_and_determinism(main_case):
    p, out = main_case
    gen = torch.Generator().manual_seed(7)
    G = torch.randn(MAIN["B"], MAIN["T"], MAIN["E"], generator=gen).to(torch.bfloat16)
    dW64, db64, bW, bb, first = check_backward(p, out, G)
    again = grads(p, out, G, accumulate=False)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])            # bit-identical run to run
    pre = (torch.randn(MAIN["E"], MAIN["C"], generator=gen), torch.randn(MAIN["E"], generator=gen))
    dW, db, _ = grads(p, out, G, accumulate=True, prefill=pre)
    assert bool(((dW.double() - pre[0].double() - dW64).abs() <= bW).all())
    assert bool(((db.double() - pre[1].double() - db64).abs() <= bb).all())
    # clear_rows = 0 leaves the gradient as it came
    _, _, g_kept = grads(p, out, G, accumulate=False, clear=False)
    assert torch.equal(g_kept, G)


def test_backward_reads_fp32_gradients_too(main_case):
    p, out = main_case
    G = torch.randn(MAIN["B"], MAIN["T"], MAIN["E"], generator=torch.Generator().manual_seed(8)).to(torch.bfloat16).float()
    check_backward(p, out, G, " fp32")


def test_forward_is_bit_identical_from_run_to_run(main_case):
    p, out = main_case
    assert torch.equal(run_forward(p, "interleaved")["emb"], out["emb"])


@pytest.mark.parametrize("counts,rows", [([0, 0], [[], []]), ([0, 1], [[], [17]])])
def test_backward_no_image_and_one_image(counts, rows):
    p = problem(3, B=2, T=64, N=3, C=32, E=128, counts=counts, rows=rows)
    out = run_forward(p, "interleaved")
    G = torch.randn(2, 64, 128, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    check_backward(p, out, G)
    if sum(counts) == 0:
        dW, db, g_after = grads(p, out, G, accumulate=False)
        assert float(dW.abs().max()) == 0.0 and float(db.abs().max()) == 0.0 and torch.equal(g_after, G)   # exact zeros
        pre = (torch.randn(128, 32), torch.randn(128))
        dW, db, _ = grads(p, out, G, accumulate=True, prefill=pre)
        assert torch.equal(dW, pre[0]) and torch.equal(db, pre[1])                        # untouched


def test_invalid_arguments_are_a_status_not_a_launch():
    from msr3d_amd.model import image_tokens as it
    ids = layout(2, 64, [[3], [4]]).to(DEV)
    masks = torch.ones(2, 1, dtype=torch.bool, device=DEV)

    def call(C, E, wdtype=torch.float32):
        emb = torch.zeros(2, 64, E, dtype=torch.bfloat16, device=DEV)
        w = torch.zeros(E, C, dtype=wdtype, device=DEV)
        it._launch(emb, None, ids, torch.zeros(2, 1, C, device=DEV), masks, w, None, TOK, "interleaved")
        torch.cuda.synchronize()
        return emb
    call(32, 128)                                                        # the smallest valid shape passes
    for C, E, wd in ((48, 128, torch.float32), (32, 192, torch.float32), (32, 128, torch.bfloat16)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            call(C, E, wd)
    with pytest.raises(RuntimeError, match="invalid argument"):
        it.image_project_grad(torch.zeros(2, 64, 128, dtype=torch.bfloat16, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV),
                              torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV),
                              torch.zeros(2, 48, device=DEV), torch.zeros(128, 48, device=DEV), None)


def test_the_no_grad_entry_refuses_to_cut_a_trainable_projection_off():
    from msr3d_amd.model import image_tokens as it
    lin = torch.nn.Linear(32, 128).to(DEV)
    emb = torch.zeros(2, 64, 128, dtype=torch.bfloat16, device=DEV)
    ids = layout(2, 64, [[3], [4]]).to(DEV)
    with pytest.raises(RuntimeError, match="no autograd"):
        it.project_scatter_images_(emb, None, ids, torch.zeros(2, 1, 32, device=DEV), torch.ones(2, 1, dtype=torch.bool, device=DEV),
                                   lin, TOK)


def test_autograd_node_returns_the_kernel_gradients_and_zeros_without_images():
    """Outside the flat-gradient engine the node hands dW / db to autograd; a batch without images gives ZERO gradients, not
    None."""
    from msr3d_amd.model import image_tokens as it
    p = problem(6, B=2, T=64, N=3, C=32, E=128, counts=[2, 1], rows=[[4, 5], [63]])
    dest, src, _, _ = reference(p, "interleaved")
    lin = torch.nn.Linear(32, 128).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(p["W"])
        lin.bias.copy_(p["b"])
    G = torch.randn(2, 64, 128, generator=torch.Generator().manual_seed(10)).to(torch.bfloat16)
    emb = it.project_scatter_images_train_(p["emb"].to(DEV), None, p["ids"].to(DEV), p["fts"].to(DEV), p["masks"].to(DEV), lin, TOK)
    emb.backward(G.to(DEV))
    g64, f64 = G.reshape(-1, 128)[dest].double(), p["fts"].reshape(-1, 32)[src].double()
    assert bool(((lin.weight.grad.cpu().double() - g64.T @ f64).abs() <= 4 * 5 * U * (g64.abs().T @ f64.abs())).all())
    assert bool(((lin.bias.grad.cpu().double() - g64.sum(0)).abs() <= 4 * 5 * U * g64.abs().sum(0)).all())
    lin.zero_grad(set_to_none=True)
    none = torch.zeros_like(p["masks"]).to(DEV)
    emb = it.project_scatter_images_train_(p["emb"].to(DEV), None, p["ids"].to(DEV), p["fts"].to(DEV), none, lin, TOK)
    emb.backward(G.to(DEV))
    assert lin.weight.grad is not None and float(lin.weight.grad.abs().max()) == 0.0 and float(lin.bias.grad.abs().max()) == 0.0
