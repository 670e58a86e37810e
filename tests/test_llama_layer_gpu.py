"""One LoRA-Llama decoder layer (msr3d_amd/llm/decoder.py, csrc/llm_layer.hip, csrc/lora_linear.hip) against
the reference stack's own output: tests/golden/llama_layer_seed0.npz was produced by transformers'
LlamaDecoderLayer + peft's LoRA formula in float32 on bf16-rounded operands
(tests/golden/make_golden_llama_layer.py; /root/reference/model/msr3d/msr3d.py:103-112, 409-415).  The HIP
layer stores every intermediate in bf16 (the reference runs under bf16 autocast, too): tolerance 2e-2 rel-L2
on the output and on every gradient.  Plus each row-local kernel against float64 on its own."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _layer(g):
    from msr3d_amd.llm import LoRALlamaDecoderLayer
    from tests.helpers import llama_layer_weights
    hidden, heads, inter, r, alpha, B, T = (int(v) for v in g["cfg"])
    w = llama_layer_weights(int(g["seed"]), hidden, inter, r)
    layer = LoRALlamaDecoderLayer(hidden, heads, inter, r=r, lora_alpha=alpha, rms_eps=float(g["eps"]),
                                  rope_theta=float(g["theta"]), device="cuda")
    with torch.no_grad():
        for n in NAMES:
            m = (layer.self_attn if n in layer.self_attn else layer.mlp)[n]
            m.load_base_weight(torch.from_numpy(w[n]).cuda())
            m.lora_A.weight.copy_(torch.from_numpy(w[n + ".A"]))
            m.lora_B.weight.copy_(torch.from_numpy(w[n + ".B"]))
        layer.input_layernorm_weight.copy_(torch.from_numpy(w["ln1"]))
        layer.post_attention_layernorm_weight.copy_(torch.from_numpy(w["ln2"]))
    return layer


def test_decoder_layer_matches_the_transformers_fixture():
    g = dict(np.load(os.path.join(GOLD, "llama_layer_seed0.npz")))
    layer = _layer(g)
    x = torch.from_numpy(g["x"]).cuda().to(torch.bfloat16).requires_grad_(True)
    keep = torch.from_numpy(g["keep"]).cuda()
    rows = keep.bool()
    y = layer(x, attention_mask=keep)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    want = torch.from_numpy(g["y"]).cuda()
    assert rel(y.float()[rows], want[rows]) < 2e-2
    gy = torch.from_numpy(g["gy"]).cuda() * rows[..., None]
    y.backward(gy.to(torch.bfloat16))
    assert rel(x.grad.float()[rows], torch.from_numpy(g["dx"]).cuda()[rows]) < 2e-2
    for n in NAMES:
        m = (layer.self_attn if n in layer.self_attn else layer.mlp)[n]
        assert rel(m.lora_A.weight.grad, g["dA/" + n]) < 2.5e-2, n
        assert rel(m.lora_B.weight.grad, g["dB/" + n]) < 2.5e-2, n


def test_decoder_layer_with_rank_32_pairs():
    """r = 32: q / k / v do not fit one 64-column low-rank activation (3 x 32 = 96): q and k share a product, v keeps its
    own (round 4 raised at construction).  Same values as the layer with no input groups at all."""
    from msr3d_amd.llm import LoRALlamaDecoderLayer
    torch.manual_seed(0)
    a = LoRALlamaDecoderLayer(512, 4, 768, r=32, lora_alpha=32, device="cuda")
    assert a.self_attn["q_proj"]._group is a.self_attn["k_proj"]._group is not None
    assert a.self_attn["v_proj"]._group is None and a.mlp["gate_proj"]._group is a.mlp["up_proj"]._group is not None
    b = LoRALlamaDecoderLayer(512, 4, 768, r=32, lora_alpha=32, device=None).cuda()       # built on the CPU: ungrouped
    assert b.self_attn["q_proj"]._group is None
    with torch.no_grad():
        for (_, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
            pa.normal_(0, 0.05)
            pb.copy_(pa)
        for n in NAMES:
            ma, mb = (a.self_attn if n in a.self_attn else a.mlp)[n], (b.self_attn if n in b.self_attn else b.mlp)[n]
            w = torch.randn(ma.out_features, ma.in_features, device="cuda") * 0.05
            ma.load_base_weight(w)
            mb.load_base_weight(w)
    x = (torch.randn(2, 64, 512, device="cuda") * 0.5).to(torch.bfloat16)
    outs = []
    for layer in (a, b):
        xi = x.clone().requires_grad_(True)
        y = layer(xi)
        y.float().square().sum().backward()
        outs.append((y.float(), xi.grad.float(), [p.grad.clone() for p in layer.parameters()]))
    assert rel(outs[0][0], outs[1][0]) < 1e-2 and rel(outs[0][1], outs[1][1]) < 2e-2
    for ga, gb in zip(outs[0][2], outs[1][2]):
        assert rel(ga, gb) < 2.5e-2


def test_shared_input_gradient_survives_a_second_backward_pass():
    """The members of an input group share ONE d-input buffer per backward pass (the first hands it to autograd, the others
    add into it).  A second pass over a retained graph must start with a buffer of its own: both passes give the same
    d input, equal to the sum of the members' own gradients."""
    from msr3d_amd.llm import LoRALinear
    from msr3d_amd.llm.lora import group_inputs
    torch.manual_seed(1)
    mods = [LoRALinear(256, 256, r=16, device="cuda") for _ in range(3)]
    with torch.no_grad():
        for m in mods:
            m.load_base_weight(torch.randn(256, 256, device="cuda") * 0.05)
            m.lora_B.weight.normal_(0, 0.05)
    group_inputs(mods, shared_grad=True)
    x = (torch.randn(128, 256, device="cuda") * 0.5).to(torch.bfloat16).requires_grad_(True)
    h = x * 1.0                                            # (a non-leaf input, as the norm's output is)
    loss = sum(m(h).float().square().sum() for m in mods)
    loss.backward(retain_graph=True)
    g1 = x.grad.clone()
    x.grad = None
    loss.backward()
    g2 = x.grad.clone()
    assert torch.equal(g1, g2) and float(g1.float().abs().sum()) > 0
    # against members that each return their own gradient (no sharing declared)
    ref = [LoRALinear(256, 256, r=16, device="cuda") for _ in range(3)]
    with torch.no_grad():
        for m, q in zip(mods, ref):
            q.load_base_weight(m.weight)
            q.lora_A.weight.copy_(m.lora_A.weight)
            q.lora_B.weight.copy_(m.lora_B.weight)
    xr = x.detach().clone().requires_grad_(True)
    sum(q(xr * 1.0).float().square().sum() for q in ref).backward()
    assert rel(g1.float(), xr.grad.float()) < 2e-2


def _call(name, *a):
    from msr3d_amd import _lib
    rc = getattr(_lib.load(), name)(*a)
    assert rc == 0, (name, rc)


def _p(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


@pytest.mark.parametrize("M,D", [(2304, 4096), (37, 512), (130, 5120)])
def test_rmsnorm_forward_backward_vs_float64(M, D):
    import ctypes
    from msr3d_amd import _lib
    torch.manual_seed(M)
    st = _lib.current_stream_ptr(torch.device("cuda"))
    x = torch.randn(M, D, device="cuda").bfloat16()
    d = torch.randn(M, D, device="cuda").bfloat16()
    w = (1 + 0.1 * torch.randn(D, device="cuda")).bfloat16()
    s, y = torch.empty_like(x), torch.empty_like(x)
    rstd = torch.empty(M, device="cuda")
    _call("msr3d_rmsnorm_fwd", M, D, _p(x), _p(d), _p(w), ctypes.c_float(1e-6), _p(s), _p(y), _p(rstd), st)
    sd = (x.float() + d.float()).bfloat16().double()
    assert torch.equal(s.double(), sd)
    r = torch.rsqrt(sd.pow(2).mean(-1, keepdim=True) + 1e-6)
    want = w.double() * (sd * r).bfloat16().double()
    assert rel(y, want) < 3e-3 and rel(rstd, r.squeeze(-1)) < 1e-5
    dy = torch.randn(M, D, device="cuda").bfloat16()
    dres = torch.randn(M, D, device="cuda").bfloat16()
    dx = torch.empty_like(x)
    _call("msr3d_rmsnorm_bwd", M, D, _p(dy), _p(s), _p(w), _p(rstd), _p(dres), _p(dx), st)
    sr = sd.clone().requires_grad_(True)
    (w.double() * sr * torch.rsqrt(sr.pow(2).mean(-1, keepdim=True) + 1e-6) * dy.double()).sum().backward()
    assert rel(dx, sr.grad + dres.double()) < 4e-3


def test_rope_is_the_reference_rotation_and_its_transpose():
    from msr3d_amd import _lib
    from msr3d_amd.llm.decoder import rope_tables
    B, T, H, D = 2, 96, 4, 128
    st = _lib.current_stream_ptr(torch.device("cuda"))
    x = torch.randn(B, T, H, D, device="cuda").bfloat16()
    cos, sin = rope_tables(T, D, 10000.0, "cuda")
    y = x.clone()
    _call("msr3d_rope_inplace", B, T, H, D, _p(y), _p(cos), _p(sin), 0, st)
    xd = x.double()
    rot = torch.cat([-xd[..., D // 2:], xd[..., :D // 2]], -1)
    want = xd * cos.double()[None, :, None] + rot * sin.double()[None, :, None]
    assert rel(y, want) < 3e-3
    g = torch.randn_like(x)
    gt = g.clone()
    _call("msr3d_rope_inplace", B, T, H, D, _p(gt), _p(cos), _p(sin), 1, st)
    assert abs(float((gt.double() * xd).sum() - (g.double() * want).sum())) < 2e-2 * float((g.double() * want).abs().sum()) ** 0.5 + 1.0
    # every launch shape: heads in groups of four (above), single heads (H = 3), the pair-per-thread kernel (D = 24), and
    # two tensors in one launch == one after the other
    for Bx, Tx, Hx, Dx in ((1, 64, 3, 64), (2, 10, 2, 24), (1, 32, 8, 128)):
        xa = torch.randn(Bx, Tx, Hx, Dx, device="cuda").bfloat16()
        xb = torch.randn(Bx, Tx, Hx, Dx, device="cuda").bfloat16()
        cs, sn = rope_tables(Tx, Dx, 10000.0, "cuda")
        for tr in (0, 1):
            one_a, one_b, two_a, two_b = xa.clone(), xb.clone(), xa.clone(), xb.clone()
            _call("msr3d_rope_inplace", Bx, Tx, Hx, Dx, _p(one_a), _p(cs), _p(sn), tr, st)
            _call("msr3d_rope_inplace", Bx, Tx, Hx, Dx, _p(one_b), _p(cs), _p(sn), tr, st)
            _call("msr3d_rope_inplace2", Bx, Tx, Hx, Dx, _p(two_a), _p(two_b), _p(cs), _p(sn), tr, st)
            assert torch.equal(one_a, two_a) and torch.equal(one_b, two_b)
            xd2 = xa.double()
            rot2 = torch.cat([-xd2[..., Dx // 2:], xd2[..., :Dx // 2]], -1)
            sgn = -1.0 if tr else 1.0
            assert rel(one_a, xd2 * cs.double()[None, :, None] + sgn * rot2 * sn.double()[None, :, None]) < 3e-3


def test_causal_softmax_and_swiglu_vs_float64():
    from msr3d_amd import _lib
    st = _lib.current_stream_ptr(torch.device("cuda"))
    n = 4096 * 24
    gte, up, dh = (torch.randn(n, device="cuda").bfloat16() for _ in range(3))
    out, dg, du = torch.empty_like(gte), torch.empty_like(gte), torch.empty_like(gte)
    _call("msr3d_swiglu_fwd", n, _p(gte), _p(up), _p(out), st)
    gd = gte.double().requires_grad_(True)
    ud = up.double().requires_grad_(True)
    ref = torch.nn.functional.silu(gd) * ud
    assert rel(out, ref) < 4e-3
    _call("msr3d_swiglu_bwd", n, _p(gte), _p(up), _p(dh), _p(dg), _p(du), st)
    ref.backward(dh.double())
    assert rel(dg, gd.grad) < 4e-3 and rel(du, ud.grad) < 4e-3


def test_batched_gemm_and_transpose():
    import ctypes
    from msr3d_amd import _lib
    B, T, H, D = 2, 192, 3, 128
    HD = H * D
    st = _lib.current_stream_ptr(torch.device("cuda"))
    q = torch.randn(B, T, H, D, device="cuda").bfloat16()
    k = torch.randn(B, T, H, D, device="cuda").bfloat16()
    S = torch.empty(B, H, T, T, device="cuda")
    _call("msr3d_bf16_gemm_batched", B, H, T, T, D, _p(q), HD, T * HD, D, _p(k), HD, T * HD, D, _p(S), T, H * T * T, T * T, 1,
          ctypes.c_float(0.5), st)
    want = 0.5 * torch.einsum("bthd,bshd->bhts", q.double(), k.double())
    assert rel(S, want) < 1e-5


@pytest.mark.parametrize("M", [2304, 2000])
def test_projection_gemm_throughput(M):
    """The frozen 4096 x 4096 projection with its LoRA pair: report TFLOP/s (275 = 11 % of 2.5 PF)."""
    from msr3d_amd.llm import LoRALinear
    K = N = 4096
    lin = LoRALinear(K, N, r=16, device="cuda")
    lin.load_base_weight(torch.randn(N, K, device="cuda") / 64)
    x = torch.randn(M, K, device="cuda").bfloat16()
    with torch.no_grad():
        for _ in range(20):          # (a cold process: clocks and the first launches' lazy setup)
            lin(x)
        torch.cuda.synchronize()
        ms = float("inf")
        for _ in range(3):           # best of three windows: a stray allocator / clock hiccup must not fail the bound
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                lin(x)
            e1.record()
            torch.cuda.synchronize()
            ms = min(ms, e0.elapsed_time(e1) / 10)
    tf = 2.0 * M * N * (K + 32 + 128) / (ms * 1e-3) / 1e12
    print(f"\nLoRALinear forward M={M} K=N=4096: {ms * 1e3:.1f} us = {tf:.0f} TFLOP/s = {tf / 2500:.1%} of the bf16 dense peak")
    assert tf > 150


@pytest.mark.parametrize("B,T,H,D,pad", [(2, 192, 3, 128, (0, 37)), (1, 576, 2, 128, (60,)), (2, 128, 4, 64, (0, 0)),
                                          (3, 64, 1, 64, (5, 0, 63))])
def test_fused_attention_forward_backward_vs_float64(B, T, H, D, pad):
    """msr3d_attn_fwd / _bwd (csrc/llm_attn.hip) == softmax(q k^T / sqrt(D) + causal + key padding) v in float64 on the
    same bf16 operands: output, log-sum-exp, dq / dk / dv; left-padded sequences (rows with no visible key give zeros and
    take no gradient); bit-identical run to run (every output row has one owner)."""
    import ctypes
    import math

    from msr3d_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + T + D)
    mk = lambda: (torch.randn(B, T, H, D, generator=g, device="cuda") * 1.5).to(torch.bfloat16)      # noqa: E731
    q, k, v, do = mk(), mk(), mk(), mk()
    keep = torch.ones(B, T, dtype=torch.uint8, device="cuda")
    for b, n in enumerate(pad):
        keep[b, :n] = 0
    scale = 1.0 / math.sqrt(D)
    st = _lib.current_stream_ptr(torch.device("cuda"))
    HD = H * D

    def run():
        out = torch.empty(B, T, HD, dtype=torch.bfloat16, device="cuda")
        lse = torch.empty(B, H, T, device="cuda")
        _call("msr3d_attn_fwd", B, T, H, D, _p(q), _p(k), _p(v), HD, _p(keep), ctypes.c_float(scale), _p(out), _p(lse), st)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        delta = torch.empty_like(lse)
        _call("msr3d_attn_bwd", B, T, H, D, _p(q), _p(k), _p(v), _p(out), _p(do), HD, _p(keep), ctypes.c_float(scale),
              _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), st)
        torch.cuda.synchronize()
        return out, lse, dq, dk, dv

    out, lse, dq, dk, dv = run()
    qd, kd, vd = (t.double().permute(0, 2, 1, 3).requires_grad_(True) for t in (q, k, v))      # (B, H, T, D)
    S = (qd @ kd.transpose(-1, -2)) * scale
    vis = torch.tril(torch.ones(T, T, dtype=torch.bool, device="cuda"))[None, None] & keep.bool()[:, None, None, :]
    Pm = torch.softmax(S.masked_fill(~vis, float("-inf")), -1).nan_to_num(0.0)
    ref = (Pm @ vd).permute(0, 2, 1, 3).reshape(B, T, HD)
    assert rel(out, ref) < 4e-3
    dead = ~vis.any(-1)                                                  # (B, 1, T) rows with no visible key
    assert float(out.float().view(B, T, H, D)[dead[:, 0]].abs().max() if dead.any() else 0.0) == 0.0
    want_lse = torch.logsumexp(S.masked_fill(~vis, float("-inf")), -1) / math.log(2.0)
    live = ~dead.expand(B, H, T)
    assert float((lse.double() - want_lse)[live].abs().max()) < 2e-3
    assert bool(torch.isinf(lse[~live]).all())
    ref.backward(do.double().reshape(B, T, HD))
    for got, want in ((dq, qd.grad), (dk, kd.grad), (dv, vd.grad)):
        assert rel(got, want.permute(0, 2, 1, 3)) < 8e-3
    again = run()
    for x, y in zip((out, lse, dq, dk, dv), again):
        assert torch.equal(x, y)
    # no key mask at all (NULL) == a mask of ones
    if not any(pad):
        out2 = torch.empty_like(out)
        lse2 = torch.empty_like(lse)
        _call("msr3d_attn_fwd", B, T, H, D, _p(q), _p(k), _p(v), HD, _p(None), ctypes.c_float(scale), _p(out2), _p(lse2), st)
        dq2, dk2, dv2, dl2 = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty_like(lse)
        _call("msr3d_attn_bwd", B, T, H, D, _p(q), _p(k), _p(v), _p(out2), _p(do), HD, _p(None), ctypes.c_float(scale),
              _p(lse2), _p(dl2), _p(dq2), _p(dk2), _p(dv2), st)
        torch.cuda.synchronize()
        for x, y in zip((out, lse, dq, dk, dv), (out2, lse2, dq2, dk2, dv2)):
            assert torch.equal(x, y)
    # refused shapes: T not a multiple of 64, head size 96
    assert _lib.load().msr3d_attn_fwd(B, T - 8, H, D, _p(q), _p(k), _p(v), HD, _p(keep), ctypes.c_float(scale), _p(out),
                                      _p(lse), st) == -22
    assert _lib.load().msr3d_attn_fwd(B, T, H, 96, _p(q), _p(k), _p(v), HD, _p(keep), ctypes.c_float(scale), _p(out),
                                      _p(lse), st) == -22
