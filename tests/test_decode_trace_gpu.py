"""The launch sequence of the decoding engine (msr3d_amd/llm: CachedDecoder's prefill, expand, step and score), pinned for
every products source (lora="separate" | "merged", weights="e4m3") and both cache layouts: recorded at the library's door
(`_lib._Entry.fn`, as tests/test_schedule_trace_gpu.py records the prompter schedule) and compared with the sequences
written below -- every launch's entry name and its leading integer arguments (rows, widths, lengths, heads), for the
skinny products M, K, R, njobs, swiglu.  A change of the engine's host code that moves, drops, adds or resizes a launch
fails here by name.

`run_case()` also returns every launch's full argument list with pointers replaced by (buffer, byte offset) against the
cache's, the stack's and the inputs' tensors, for comparing two versions of the host code launch by launch (same
library, same arguments: same computation)."""
import functools

import pytest
import torch

from tests.generate_helpers import CFG, gpu_stack, prompt
from tests.test_schedule_trace_gpu import _label, _snap

pytestmark = pytest.mark.gpu

NL, HID, H, INTER, V, RANK = (CFG[k] for k in ("layers", "hidden", "heads", "inter", "vocab", "r"))
D = HID // H
T, TP = 24, 64                                    # prompt(0)'s slots, and what the prefill pads them to (one key tile)
NEW, BEAMS = 4, 5                                 # reserve(5, 4)
PAIRS = 7 * NL                                    # LoRA pairs of the stack: the jobs of a shadows or merge launch

RMS, SWIGLU = "msr3d_rmsnorm_fwd", "msr3d_swiglu_fwd"
R_ROW, R_ROW_Q = "msr3d_bf16_gemm_skinny", "msr3d_bf16_gemm_skinny_quant"
GEMM, GEMM_FP8, SKINNY_FP8 = "msr3d_bf16_gemm_lowrank", "msr3d_fp8_gemm_lowrank", "msr3d_fp8_skinny_lowrank"
SKINNY = ("msr3d_bf16_skinny_lowrank", "msr3d_bf16_skinny_lowrank_wide")      # up to 32 live rows | 33 .. 64
JOBS_AT = {SKINNY[0]: (7, 9), SKINNY[1]: (7, 9), SKINNY_FP8: (8, 10)}         # where njobs and swiglu stand


# ---------------------------------------------------------------------------------------------- recording
def _coarse(name, args):
    """(name, the integer arguments in front of the first pointer) + (njobs, swiglu) of a skinny product."""
    lead = []
    for a in args:
        if not isinstance(a, int):
            break
        lead.append(a)
    return (name, *lead, *(args[i] for i in JOBS_AT.get(name, ())))


def record(fn):
    """fn() with every library launch recorded -> [(entry name, [argument as plain data])]."""
    from msr3d_amd import _lib
    lib = _lib.load()
    entries = [e for e in (getattr(lib, n) for n in _lib._SIGNATURES) if isinstance(e, _lib._Entry)]
    saved = [e.fn for e in entries]
    trace = []

    def wrap(e, call):
        types = _lib._SIGNATURES[e.name]

        def f(*a):
            trace.append((e.name, [_snap(x, t) for x, t in zip(a, types)]))
            return call(*a)
        return f
    try:
        for e, call in zip(entries, saved):
            e.fn = wrap(e, call)
        fn()
    finally:
        for e, call in zip(entries, saved):
            e.fn = call
    torch.cuda.synchronize()
    return trace


def _buffers(net, eng, inputs):
    """The tensors a launch may point into, by name: the inputs, the cache's, the engine's tables, the stack's."""
    from msr3d_amd.llm import LoRALinear
    out = {"in:" + k: t for k, t in inputs.items()}
    for k, v in vars(eng.cache).items():
        for j, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(t, torch.Tensor):
                out[f"cache:{k}{j}"] = t
    for j, t in enumerate(getattr(eng, "_tables", None) or ()):
        if isinstance(t, torch.Tensor):
            out[f"rope{j}"] = t
    for n, m in net.named_modules():
        if isinstance(m, LoRALinear):
            if m._group is not None and m._group["mods"][0] is m:         # (before the members' slices of it)
                out[f"net:{n}.a_cat"] = m._group["a_cat"]
            for j, t in enumerate(m._shadow or ()):
                out[f"net:{n}.shadow{j}"] = t
            for k in ("weight_q", "weight_scale"):
                if getattr(m, k) is not None:
                    out[f"net:{n}.{k}"] = getattr(m, k)
            if net._merged is not None:
                out[f"net:{n}.merged"] = net._merged[1][m]
    out.update({"net:" + n: t for n, t in list(net.named_parameters()) + list(net.named_buffers())})
    return out


# ---------------------------------------------------------------------------------------------- the models
@functools.lru_cache(maxsize=None)
def _grouped(base):
    return gpu_stack(0, base=base)


@functools.lru_cache(maxsize=None)
def _ungrouped(base):
    """A stack built without a device and moved: its modules have no input group (LoRALlamaDecoderLayer groups q | k | v
    and gate | up only when it is built on a cuda device)."""
    from msr3d_amd.llm import LoRALinear, LoRALlamaStack
    c = CFG
    net = LoRALlamaStack(c["layers"], c["hidden"], c["heads"], c["inter"], c["vocab"], r=c["r"], lora_alpha=c["alpha"],
                         rms_eps=c["eps"], rope_theta=c["theta"], base=base)
    gen = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for n, b in net.named_buffers():
            if b.dim() == 2:
                b.copy_(torch.randn(b.shape, generator=gen) * b.shape[1] ** -0.5)
    net = net.cuda()
    for m in net.modules():
        if isinstance(m, LoRALinear):
            assert m._group is None
            m._sync_weight_t()                    # (the transposed and e4m3 images of the moved weight: not the walk's)
    return net, _grouped("bf16")[1]


def _engine(kind, layout, grouped=True):
    from msr3d_amd.llm.generate import CachedDecoder
    base = "fp8" if kind == "e4m3" else "bf16"
    net, emb = _grouped(base) if grouped else _ungrouped(base)
    for m in net._pairs():                        # every case starts on stale images: one shadows or merge launch
        m.invalidate_shadows()
    kw = dict(weights="e4m3") if kind == "e4m3" else dict(lora=kind)
    return net, emb, CachedDecoder(net, prompt_cache=layout, **kw)


# ---------------------------------------------------------------------------------------------- the walks
def _walk_beams(kind, layout, B, per=BEAMS, grouped=True, reorder=True):
    """reserve, prefill, expand, a step, a step whose beam_idx permutes the rows inside every prompt."""
    net, emb, eng = _engine(kind, layout, grouped)
    x, keep = prompt(0, B=B)
    g = torch.arange(B * per)
    ins = dict(x=x.cuda(), keep=keep.cuda(), tok=emb[torch.arange(B * per).cuda() + 3].contiguous(),
               beam_idx=((g // per) * per + torch.tensor([1, 0, 3, 2, 4])[g % per]).cuda() if per == BEAMS else None)

    def walk():
        eng.reserve(per, NEW)
        eng.prefill(ins["x"], ins["keep"])
        eng.expand(per)
        eng.step(ins["tok"])
        if reorder:
            eng.step(ins["tok"], ins["beam_idx"])
    return net, eng, ins, walk


def _walk_score(kind, max_rows):
    """reserve(1, 0), prefill(positions="arange") with B = 3, `score` of C = 3 candidates of S = 5 tokens."""
    net, emb, eng = _engine(kind, "rows")
    x, keep = prompt(0, B=3)
    ids = (torch.arange(3 * 3 * 5) % 7 + 3).view(3, 3, 5)
    tk = torch.ones(3, 3, 5, dtype=torch.bool)
    tk[:, 1, 3:] = False
    ins = dict(x=x.cuda(), keep=keep.cuda(), suffix=emb[ids.cuda()].contiguous(), suffix_keep=tk.cuda())

    def walk():
        eng.reserve(1, 0)
        eng.prefill(ins["x"], ins["keep"], positions="arange")
        if max_rows is None:
            eng.score(ins["suffix"], ins["suffix_keep"])
        else:
            eng.score(ins["suffix"], ins["suffix_keep"], max_rows=max_rows)
    return net, eng, ins, walk


# ---------------------------------------------------------------------------------------------- the sequences
def _entry(M):
    return SKINNY[0] if M <= 32 else SKINNY[1]


def _skinny(kind, M, K, Ns, grouped=True, swiglu=False):
    """The weight-stream products of len(Ns) projections of the same (M, K) activations: the group's r-row launch (none on
    merged planes), then ONE launch for its members.  Members without a shared input group: one such pair each, and a
    stand-alone SwiGLU launch where gate | up would have carried the epilogue."""
    n = len(Ns)
    if n > 1 and not grouped:
        return [r for N in Ns for r in _skinny(kind, M, K, [N])] + ([(SWIGLU, M * Ns[0])] if swiglu else [])
    if kind == "separate":
        return [(R_ROW, M, RANK * n, K), (_entry(M), M, K, 64, n, int(swiglu))]
    if kind == "merged":
        return [(_entry(M), M, K, 0, n, int(swiglu))]
    return [(R_ROW_Q, M, RANK * n, K), (SKINNY_FP8, M, K, 64, n, int(swiglu))]


def _wide(kind, M, K, Ns, grouped=True, swiglu=False):
    """The same products in prefill and `score`: the modules' own forward (one r-row product per input group, one tiled
    GEMM per member, SwiGLU as a launch); merged: one R = 0 GEMM per member; e4m3 below 128 rows: slabs of at most 64
    rows on the skinny kernel."""
    if kind == "e4m3" and M < 128:
        return [r for s in range(0, M, 64) for r in _skinny(kind, min(64, M - s), K, Ns, grouped, swiglu)]
    act = [(SWIGLU, M * Ns[0])] if swiglu else []
    if kind == "merged":
        return [(GEMM, M, N, K, 0) for N in Ns] + act
    if kind == "separate":
        r_row, gemms = R_ROW, [(GEMM, M, N, K, 64) for N in Ns]
    else:
        assert grouped or len(Ns) == 1            # (no case here runs ungrouped e4m3 modules at 128 rows or more)
        r_row, gemms = R_ROW_Q, [(GEMM_FP8, M, N, K) for N in Ns]
    if grouped:
        return [(r_row, M, RANK * len(Ns), K)] + gemms + act
    return [r for gm in gemms for r in ((r_row, M, RANK, K), gm)] + act


def _stack(kind, products, M, M_last, attend, grouped=True):
    """decoder_stack: per layer the norm, q | k | v, `attend`, o, the norm, gate | up, down -- the last layer's second
    half and the final norm on the M_last rows the head reads."""
    out = []
    for i in range(NL):
        m2 = M_last if i == NL - 1 else M
        out += ([(RMS, M, HID)] + products(kind, M, HID, [HID] * 3, grouped) + attend + products(kind, M, HID, [HID])
                + [(RMS, m2, HID)] + products(kind, m2, HID, [INTER] * 2, grouped, True) + products(kind, m2, INTER, [HID]))
    return out + [(RMS, M_last, HID)]


def _refresh(kind):
    return [("msr3d_lora_merge", PAIRS)] if kind == "merged" else [("msr3d_lora_shadows", PAIRS)]


def _prefill(kind, B, grouped=True):
    attend = [("msr3d_rope_positions", B, TP, H, D), ("msr3d_attn_fwd", B, TP, H, D)]
    return _refresh(kind) + _stack(kind, _wide, B * TP, B, attend, grouped) + [(GEMM, B, V, HID, 0)]


def _step(kind, layout, B, per, new=NEW, grouped=True, reorder=False):
    N = B * per
    if layout == "shared":
        t = new
        attend = [("msr3d_rope_kv_append", N, H, D, new), ("msr3d_attn_decode_shared", B, per, T, new, H, D)]
    else:
        t = T + new
        attend = [("msr3d_rope_kv_append", N, H, D, t), ("msr3d_attn_decode", N, t, H, D)]
    return ([("msr3d_kv_reorder", 2 * NL, N, t, HID)] if reorder else []) + \
        _stack(kind, _skinny, N, N, attend, grouped) + [(_entry(N), N, HID, 0, 1, 0)]


def _score(kind, B, C, S, max_rows):
    Sp, out = 16, []
    per = max(1, max_rows // (B * Sp))
    for c0 in range(0, C, per):
        Cc = min(per, C - c0)
        N = B * Cc
        attend = [("msr3d_rope_positions", N, Sp, H, D), ("msr3d_attn_prefix_fwd", B, Cc, Sp, T, H, D)]
        out += _stack(kind, _wide, N * Sp, N * S, attend) + [(GEMM, N * S, V, HID, 0)]
    return out


def _beams(kind, layout, B):
    return _prefill(kind, B) + _step(kind, layout, B, BEAMS) + _step(kind, layout, B, BEAMS, reorder=True)


# id: (the walk, the expected sequence)
CASES = {}
for _kind, _layout in (("separate", "rows"), ("separate", "shared"), ("merged", "rows"), ("merged", "shared"),
                       ("e4m3", "rows"), ("e4m3", "shared")):
    CASES[f"beams-{_kind}-{_layout}"] = (functools.partial(_walk_beams, _kind, _layout, 1), _beams(_kind, _layout, 1))
for _kind, _layout in (("separate", "rows"), ("merged", "shared")):                # 40 live rows: the wide bf16 entry
    CASES[f"beams40-{_kind}-{_layout}"] = (functools.partial(_walk_beams, _kind, _layout, 8), _beams(_kind, _layout, 8))
# one row a prompt: nothing to share, the rows layout
CASES["shared-one_row_a_prompt"] = (functools.partial(_walk_beams, "separate", "shared", 2, per=1, reorder=False),
                                    _prefill("separate", 2) + _step("separate", "rows", 2, 1))
for _kind in ("separate", "merged", "e4m3"):
    # 3 x 3 x 16 = 144 suffix rows in one chunk | chunks of 96 and 48 rows (under e4m3: slabs of 64 + 32, and 48)
    CASES[f"score-{_kind}"] = (functools.partial(_walk_score, _kind, None),
                               _prefill(_kind, 3) + _score(_kind, 3, 3, 5, 8192))
    CASES[f"score96-{_kind}"] = (functools.partial(_walk_score, _kind, 96),
                                 _prefill(_kind, 3) + _score(_kind, 3, 3, 5, 96))
for _kind in ("separate", "merged", "e4m3"):
    # modules without an input group: a product pair per projection, gate and up apart and msr3d_swiglu_fwd after them
    CASES[f"ungrouped-{_kind}"] = (functools.partial(_walk_beams, _kind, "rows", 1, per=1, grouped=False, reorder=False),
                                   _prefill(_kind, 1, grouped=False) + _step(_kind, "rows", 1, 1, grouped=False))


def run_case(name):
    """-> (engine, coarse records, labelled full trace) of one case of CASES."""
    net, eng, ins, walk = CASES[name][0]()
    trace = record(walk)
    return eng, [_coarse(n, a) for n, a in trace], _label(trace, _buffers(net, eng, ins))


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_of_the_engine(name):
    want = CASES[name][1]
    eng, got, full = run_case(name)
    assert len(full) == len(got)
    assert eng.cache.layout == ("shared" if name.endswith("-shared") else "rows")
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i}: {g} where {w} is expected\n" + "\n".join(map(str, got))
    assert len(got) == len(want), "\n".join(map(str, got[len(want):]))


def test_the_sequences_show_what_they_are_for():
    """The cases differ where the issue says they must (read off the pinned sequences, no launch)."""
    names = lambda k: [r[0] for r in CASES[k][1]]                                   # noqa: E731
    assert SKINNY[0] in names("beams-separate-rows") and SKINNY[1] not in names("beams-separate-rows")
    assert SKINNY[1] in names("beams40-separate-rows") and SKINNY[0] not in names("beams40-separate-rows")
    assert R_ROW not in names("beams-merged-rows") and R_ROW_Q not in names("beams-merged-shared")
    assert GEMM_FP8 in names("score-e4m3")
    slabs = [r[1] for r in _score("e4m3", 3, 3, 5, 96) if r[0] == SKINNY_FP8 and r[2:] == (HID, 64, 3, 0)]
    assert slabs == [64, 32, 64, 32, 48, 48] and GEMM_FP8 not in [r[0] for r in _score("e4m3", 3, 3, 5, 96)]
    for kind in ("separate", "merged", "e4m3"):
        one, two = _step(kind, "rows", 1, 1), _step(kind, "rows", 1, 1, grouped=False)
        assert names(f"ungrouped-{kind}").count(SWIGLU) == 2 * NL and SWIGLU not in [r[0] for r in one]
        assert sum(r[-1] for r in one if r[0] in JOBS_AT) == NL and sum(r[-1] for r in two if r[0] in JOBS_AT) == 0
