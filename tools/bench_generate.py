"""Times KV-cached decoding (msr3d_amd/llm/generate.py) at Vicuna-7B layer shapes with random weights: the prefill and one
decode step at N live rows x cache length, against (a) the only way to get a token without a cache --
`LoRALlamaStack.logits(..., from_position=T-1)` on the 64-padded prefix, same process, alternating -- and (b) the
streaming floor: bytes of weights + cache a step must read / 6.29 TB/s (the rate a streaming copy reaches on an MI355X).
Device events around every repeat (warm-up first, >= 20 repeats): median and spread.  Prints one JSON line.

    python tools/bench_generate.py [--layers 4] [--repeats 20] [--rows 1,5,20,32,40,64] [--lengths 128,320,576]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_generate.py --profile 5x320      # per-kernel, own run
    python tools/bench_generate.py --sample      # the draw kernel beside the select kernel and a decode step
    python tools/bench_generate.py --lora both   # + the step on merged weights (lora="merged"), alternating with the
                                                 #   separate one; the merge launch; launches per step; the fresh-call cost
    python tools/bench_generate.py --prompt-cache both   # a BEAM step (5 rows a prompt, a reorder in it) under the rows
                                                 #   layout and under prompt_cache="shared", alternating; bytes of either
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_generate.py --prompt-cache shared --profile 20x576
    python tools/bench_generate.py --weights both   # the step of a base="fp8" stack on its e4m3 weights (weights="e4m3")
                                                 #   beside the bf16 stack's, alternating; the four projection launches of a
                                                 #   layer one by one against their streaming floors
    python tools/bench_generate.py --kv both [--prompt-cache shared] [--lora merged]   # the step on the bf16 and on the
                                                 #   e4m3 key / value cache (kv="e4m3"), alternating; the attention, append
                                                 #   and reorder launches of each against the attention's streaming floor
    python tools/bench_generate.py --loop both      # whole TOKENS (select + bookkeeping + step, a beam reorder in it) under
                                                 #   search(loop="host") and loop="device" (graph replays), alternating;
                                                 #   the capture's cost per group; the `poll` sweep; --layers-once 32 adds
                                                 #   one cell on a 32-layer stack
    python tools/bench_generate.py --step both --lora merged [--loop host|device|both]   # whole tokens under step="split"
                                                 #   and step="fused", alternating call by call; the fused products' launches
                                                 #   beside the split launches they replace; --layers-once 32 as above
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from msr3d_amd import _lib  # noqa: E402
from msr3d_amd.llm import LoRALlamaStack  # noqa: E402
from msr3d_amd.llm.generate import CachedDecoder  # noqa: E402

HIDDEN, HEADS, INTER, VOCAB = 4096, 32, 11008, 32000
COPY_RATE = 6.29e12


def build(layers, base="bf16"):
    net = LoRALlamaStack(layers, HIDDEN, HEADS, INTER, VOCAB, device="cuda", base=base)
    gen = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        for n, b in net.named_buffers():
            if n.endswith("weight") and b.dim() == 2:
                b.copy_(torch.randn(b.shape, generator=gen, device="cuda") * b.shape[1] ** -0.5)
        for p in net.lora_parameters():
            if p.shape[0] != 16:                      # lora_B: zeros at init; give it values so the term is live
                p.copy_(torch.randn(p.shape, generator=gen, device="cuda") * 0.02)
    return net


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return {"median_us": round(statistics.median(ts), 1), "min_us": round(ts[0], 1), "max_us": round(ts[-1], 1)}


def _stats(ts):
    ts = sorted(ts)
    return {"median_us": round(statistics.median(ts), 1), "min_us": round(ts[0], 1), "max_us": round(ts[-1], 1)}


def timed_alternating(fns, repeats, warmup=3):
    """Several callables timed in turn, repeat by repeat (what the machine does in between hits all of them alike)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[i].append(e0.elapsed_time(e1) * 1e3)
    return [_stats(t) for t in ts]


def library_launches(fn):
    """The library entries one call of fn launches, by name (the binding's census brackets every launch)."""
    sink = {}
    _lib.set_timing_sink(sink, census=True)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.set_timing_sink(None)
    return {k: len(v) for k, v in sorted(sink.items())}


def merge_cell(net, repeats):
    """The merge launch over every pair of the stack: events around the ENTRY on a table built beforehand (the entry reads
    the table back before it launches) and around llm.lora.merge_pairs, which also builds and uploads the table; the bytes
    -- 2 read + 2 written per element -- over the copy rate; a device copy of as many bytes; the host cost of a call on
    fresh planes."""
    from msr3d_amd.llm.lora import merge_pairs
    planes = net.merged_weights()
    mods = list(planes)
    arr = (_lib.LoraMergeJob * len(mods))(*[
        _lib.LoraMergeJob(m.weight.data_ptr(), m.lora_A.weight.data_ptr(), m.lora_B.weight.data_ptr(), planes[m].data_ptr(),
                          m.in_features, m.r, m.out_features, m.in_features, m.scaling, 0) for m in mods])
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    dev = tab.device
    entry, pairs = timed_alternating([
        lambda: _lib.call("msr3d_lora_merge", len(mods), _lib.ptr(tab), _lib.current_stream_ptr(dev)),
        lambda: merge_pairs(mods, [planes[m] for m in mods])], repeats)
    nbytes = sum(4 * m.in_features * m.out_features for m in mods)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy = timed(lambda: dst.copy_(src), repeats)
    del src, dst
    t0 = time.perf_counter()
    for _ in range(200):
        net.merged_weights()
    fresh = (time.perf_counter() - t0) / 200 * 1e6
    floor = nbytes / COPY_RATE * 1e6
    return {"pairs": len(mods), "bytes": nbytes, "entry": entry, "merge_pairs": pairs, "device_copy_same_bytes": copy,
            "floor_us": round(floor, 1), "floor_fraction": round(floor / entry["median_us"], 3),
            "fresh_call_host_us": round(fresh, 1)}


def step_bytes(layers, rows, length):
    per_layer = 2 * (4 * HIDDEN * HIDDEN + 3 * HIDDEN * INTER)
    cache = 2 * 2 * rows * length * HIDDEN
    return layers * (per_layer + cache) + 2 * HIDDEN * VOCAB


BEAMS = 5


def beam_bytes(layers, prompts, length, tail):
    """What the attention reads and the reorder reads + writes in one beam step at `tail` generated tokens, per layout."""
    tok = layers * 2 * HIDDEN * 2                                   # one token-row: K and V of every layer, bf16
    rows = prompts * BEAMS
    return {"rows": {"attention": rows * (length + tail) * tok, "reorder": 2 * rows * (length + tail) * tok},
            "shared": {"attention": (prompts * length + rows * tail) * tok, "reorder": 2 * rows * tail * tok}}


def prompt_cache_cells(args):
    """--prompt-cache: one decode step WITH a beam reorder in it (beam_idx rotates the rows within every prompt), 5 rows a
    prompt, under the rows layout (every row its own copy of the prompt) and under prompt_cache="shared", alternating
    repeat by repeat in one process.  A row count that is no multiple of 5 runs as the whole prompts that fit (64 -> 60).
    The cache grows by one token per repeat in both; the bytes are stated at the middle repeat."""
    net = build(args.layers)
    emb = torch.randn(VOCAB, HIDDEN, device="cuda").to(torch.bfloat16) * 0.02
    gen = torch.Generator(device="cuda").manual_seed(1)
    layouts = ["rows", "shared"] if args.prompt_cache == "both" else [args.prompt_cache]
    rows_arg = args.rows or "5,20,40,64"
    grid = [(int(r), int(t)) for r in rows_arg.split(",") for t in args.lengths.split(",")]
    if args.profile:
        grid = [tuple(int(v) for v in args.profile.split("x"))]
    warmup = 3
    out = {"bench": "generate_prompt_cache", "device": torch.cuda.get_device_name(0), "layers": args.layers, "hidden": HIDDEN,
           "heads": HEADS, "beams": BEAMS, "repeats": args.repeats, "copy_rate_TBps": COPY_RATE / 1e12, "layouts": layouts,
           "cells": []}
    for want, length in grid:
        prompts = max(1, want // BEAMS)
        rows = prompts * BEAMS
        x = (torch.randn(prompts, length, HIDDEN, generator=gen, device="cuda") * 0.5).to(torch.bfloat16)
        mask = torch.ones(prompts, length, dtype=torch.int64, device="cuda")
        tok = emb[torch.randint(0, VOCAB, (rows,), generator=gen, device="cuda")]
        g = torch.arange(rows, device="cuda")
        beam_idx = (g // BEAMS) * BEAMS + (g % BEAMS + 1) % BEAMS       # every row continues its neighbour in the prompt
        engines = []
        for layout in layouts:
            eng = CachedDecoder(net, prompt_cache=layout)
            eng.reserve(BEAMS, args.repeats + warmup + 8)
            eng.prefill(x, mask)
            eng.expand(BEAMS)
            engines.append(eng)
        fns = [lambda e=e: e.step(tok, beam_idx) for e in engines]
        if args.profile:
            for _ in range(20):
                for fn in fns:
                    fn()
            torch.cuda.synchronize()
            stats = [None] * len(fns)
        else:
            stats = timed_alternating(fns, args.repeats, warmup=warmup)
        tail = warmup + args.repeats // 2
        cell = {"live_rows": rows, "prompts": prompts, "length": length, "tail_at_middle": tail,
                "splits": _lib.load().msr3d_attn_decode_splits(rows, HEADS),
                "attention_workgroups": {"rows": rows * HEADS, "shared": prompts * HEADS}}
        nbytes = beam_bytes(args.layers, prompts, length, tail)
        weights = step_bytes(args.layers, 0, 0)
        for layout, eng, st in zip(layouts, engines, stats):
            b = nbytes[layout]
            floor = (weights + b["attention"] + b["reorder"]) / COPY_RATE * 1e6
            cell[layout] = {"step": st, "attention_bytes": b["attention"], "reorder_bytes": b["reorder"],
                            "cache_bytes": eng.cache.nbytes, "floor_us": round(floor, 1)}
            if st is not None:
                cell[layout]["floor_fraction"] = round(floor / st["median_us"], 3)
        if len(layouts) == 2 and stats[0] is not None:
            cell["shared_over_rows"] = round(stats[1]["median_us"] / stats[0]["median_us"], 3)
            if "launches" not in out:
                out["launches"] = {n: library_launches(fn) for n, fn in zip(layouts, fns)}
        out["cells"].append(cell)
        del engines, fns
    print(json.dumps(out))


PROJECTIONS = (("q|k|v", HIDDEN, 3 * HIDDEN), ("o", HIDDEN, HIDDEN), ("gate|up", HIDDEN, 2 * INTER), ("down", INTER, HIDDEN))


def projection_floor_us(weights, rows, K, N):
    """What a projection launch must stream -- the weight (codes + one f32 scale per output channel under e4m3) and the
    activations (codes + one f32 scale per row) -- over the copy rate."""
    nbytes = (N * K + 4 * N + rows * K + 4 * rows) if weights == "e4m3" else 2 * (N * K + rows * K)
    return nbytes / COPY_RATE * 1e6


def projection_launches(eng, tok, steps=5):
    """Per-launch device time of the four projection launches of a layer (q|k|v, o, gate|up, down) and of the r-row launch
    in front of each (under e4m3 the one that also quantises the activations), by the binding's census (events around
    EVERY library launch, so the step itself is slower while it runs): medians over layers and `steps` steps."""
    entry = eng.products.skinny.src.entry(tok.shape[0])          # (the engine's own choice for this many rows)
    layers = len(eng.stack.layers)
    sink = {}
    _lib.set_timing_sink(sink, census=True)
    try:
        for _ in range(steps):
            eng.step(tok)
        torch.cuda.synchronize()
    finally:
        _lib.set_timing_sink(None)
    r_row = "msr3d_bf16_gemm_skinny_quant" if eng.weights == "e4m3" else "msr3d_bf16_gemm_skinny"
    out = []
    for name in (entry, r_row):                                  # both are launched 4 a layer in the same order
        pairs = sink[name]
        per_step = len(pairs) // steps                           # (+ the head, last, on the bf16 entry)
        assert per_step in (4 * layers, 4 * layers + 1), (name, per_step)
        ts = [[] for _ in PROJECTIONS]
        for i, (e0, e1) in enumerate(pairs):
            j = i % per_step
            if j < 4 * layers:
                ts[j % 4].append(e0.elapsed_time(e1) * 1e3)
        out.append([round(statistics.median(t), 1) for t in ts])
    return out


def weights_cells(args):
    """--weights: one decode step of the bf16 stack (weights="bf16") and of a base="fp8" stack of the same shapes on its
    e4m3 weights (weights="e4m3"), alternating repeat by repeat in one process; then, in a run of its own per engine, the
    device time of each of the four projection launches of a layer against its streaming floor."""
    kinds = ["bf16", "e4m3"] if args.weights == "both" else [args.weights]
    nets = {k: build(args.layers, base="fp8" if k == "e4m3" else "bf16") for k in kinds}
    emb = torch.randn(VOCAB, HIDDEN, device="cuda").to(torch.bfloat16) * 0.02
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows_arg = args.rows or "1,5,20,64"
    grid = [(int(r), int(t)) for r in rows_arg.split(",") for t in args.lengths.split(",")]
    if args.profile:
        grid = [tuple(int(v) for v in args.profile.split("x"))]
    warmup, census_steps = 3, 5
    out = {"bench": "generate_weights", "device": torch.cuda.get_device_name(0), "layers": args.layers, "hidden": HIDDEN,
           "heads": HEADS, "inter": INTER, "vocab": VOCAB, "repeats": args.repeats, "copy_rate_TBps": COPY_RATE / 1e12,
           "weights": kinds, "projections": [p[0] for p in PROJECTIONS], "cells": []}
    for rows, length in grid:
        x = (torch.randn(1, length, HIDDEN, generator=gen, device="cuda") * 0.5).to(torch.bfloat16)
        mask = torch.ones(1, length, dtype=torch.int64, device="cuda")
        tok = emb[torch.randint(0, VOCAB, (rows,), generator=gen, device="cuda")]
        engines = []
        for k in kinds:
            eng = CachedDecoder(nets[k], weights=k)
            eng.reserve(rows, args.repeats + warmup + census_steps + 28)
            eng.prefill(x, mask)
            eng.expand(rows)
            engines.append(eng)
        fns = [lambda e=e: e.step(tok) for e in engines]
        cell = {"rows": rows, "length": length}
        if args.profile:
            for _ in range(20):
                for fn in fns:
                    fn()
            torch.cuda.synchronize()
            out["cells"].append(cell)
            continue
        stats = timed_alternating(fns, args.repeats, warmup=warmup)
        for k, eng, st in zip(kinds, engines, stats):
            launch, r_row = projection_launches(eng, tok, census_steps)
            floors = [projection_floor_us(k, rows, K, N) for _, K, N in PROJECTIONS]
            cell[k] = {"step": st, "projection_us": launch, "projection_floor_us": [round(f, 1) for f in floors],
                       "projection_floor_fraction": [round(f / t, 3) for f, t in zip(floors, launch)], "r_row_us": r_row}
        if len(kinds) == 2:
            cell["e4m3_over_bf16"] = round(stats[1]["median_us"] / stats[0]["median_us"], 3)
            cell["projection_e4m3_over_bf16"] = [round(a / b, 3) for a, b in zip(cell["e4m3"]["projection_us"],
                                                                                cell["bf16"]["projection_us"])]
            if "launches" not in out:
                out["launches"] = {k: library_launches(fn) for k, fn in zip(kinds, fns)}
        out["cells"].append(cell)
        del engines, fns
    print(json.dumps(out))


def kv_launches(eng, fn, steps=5):
    """Per-launch device time of the cache's launches in a step, by the binding's census (events around EVERY library
    launch): the attention and the append as medians over layers and `steps` steps, the reorder as the median over steps
    of a step's sum (one launch under bf16, two -- codes, exponents -- under e4m3)."""
    e4 = "_e4m3" if eng.kv == "e4m3" else ""
    attn = ("msr3d_attn_decode_shared" if eng.cache.shared else "msr3d_attn_decode") + e4
    sink = {}
    _lib.set_timing_sink(sink, census=True)
    try:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    finally:
        _lib.set_timing_sink(None)
    us = lambda pairs: [e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs]     # noqa: E731
    out = {"attention_us": round(statistics.median(us(sink[attn])), 1),
           "append_us": round(statistics.median(us(sink["msr3d_rope_kv_append" + e4])), 1)}
    if "msr3d_kv_reorder" in sink:
        t = us(sink["msr3d_kv_reorder"])
        per = len(t) // steps
        out["reorder_us"] = round(statistics.median([sum(t[i * per:(i + 1) * per]) for i in range(steps)]), 1)
        out["reorder_launches"] = per
    return out


def kv_cells(args):
    """--kv: one decode step on the bf16 cache and on the e4m3 cache (kv="e4m3"), alternating repeat by repeat in one
    process -- 1 row: one prompt, no beams; otherwise 5 rows a prompt with a beam reorder in the step (a row count that is
    no multiple of 5 runs as the whole prompts that fit: 64 -> 60) -- under --prompt-cache rows (default) or shared and
    --lora separate (default) or merged; then, in a run of its own per engine, the attention, append and reorder launches.
    Floors: the attention's K / V bytes of ONE layer (codes + exponent records under e4m3) over the copy rate."""
    kinds = ["bf16", "e4m3"] if args.kv == "both" else [args.kv]
    layout = args.prompt_cache or "rows"
    lora = "merged" if args.lora == "merged" else "separate"
    net = build(args.layers)
    emb = torch.randn(VOCAB, HIDDEN, device="cuda").to(torch.bfloat16) * 0.02
    gen = torch.Generator(device="cuda").manual_seed(1)
    grid = [(int(r), int(t)) for r in (args.rows or "1,5,20,64").split(",") for t in args.lengths.split(",")]
    if args.profile:
        grid = [tuple(int(v) for v in args.profile.split("x"))]
    warmup, census_steps = 3, 5
    out = {"bench": "generate_kv", "device": torch.cuda.get_device_name(0), "layers": args.layers, "hidden": HIDDEN,
           "heads": HEADS, "repeats": args.repeats, "copy_rate_TBps": COPY_RATE / 1e12, "kv": kinds, "prompt_cache": layout,
           "lora": lora, "cells": []}
    D = HIDDEN // HEADS
    for want, length in grid:
        beams = 1 if want < BEAMS else BEAMS
        prompts = max(1, want // beams)
        rows = prompts * beams
        x = (torch.randn(prompts, length, HIDDEN, generator=gen, device="cuda") * 0.5).to(torch.bfloat16)
        mask = torch.ones(prompts, length, dtype=torch.int64, device="cuda")
        tok = emb[torch.randint(0, VOCAB, (rows,), generator=gen, device="cuda")]
        g = torch.arange(rows, device="cuda")
        beam_idx = (g // beams) * beams + (g % beams + 1) % beams if beams > 1 else None
        engines = []
        for k in kinds:
            eng = CachedDecoder(net, lora=lora, prompt_cache=layout, kv=k)
            eng.reserve(beams, args.repeats + warmup + census_steps + 28)
            eng.prefill(x, mask)
            eng.expand(beams)
            engines.append(eng)
        fns = [lambda e=e: e.step(tok, beam_idx) for e in engines]
        cell = {"live_rows": rows, "prompts": prompts, "length": length, "shared": engines[0].cache.shared,
                "splits": _lib.load().msr3d_attn_decode_splits(rows, HEADS)}
        if args.profile:
            for _ in range(20):
                for fn in fns:
                    fn()
            torch.cuda.synchronize()
            out["cells"].append(cell)
            continue
        stats = timed_alternating(fns, args.repeats, warmup=warmup)
        tail = warmup + args.repeats + census_steps // 2               # (the census runs after the timed repeats)
        slots = (prompts * length + rows * tail) if engines[0].cache.shared else rows * (length + tail)
        for k, eng, fn, st in zip(kinds, engines, fns, stats):
            slot_bytes = 2 * (HEADS * D + eng.cache.exp_pad) if k == "e4m3" else 2 * 2 * HEADS * D     # K and V of a slot
            floor = slots * slot_bytes / COPY_RATE * 1e6
            cell[k] = {"step": st, "cache_bytes": eng.cache.nbytes, **kv_launches(eng, fn, census_steps),
                       "attention_floor_us": round(floor, 1)}
            cell[k]["attention_floor_fraction"] = round(floor / cell[k]["attention_us"], 3)
        if len(kinds) == 2:
            a, b = cell["bf16"], cell["e4m3"]
            cell["e4m3_over_bf16"] = {key: round(b[key] / a[key], 3) for key in ("attention_us", "append_us", "reorder_us",
                                                                                  "cache_bytes") if key in a}
            cell["e4m3_over_bf16"]["step"] = round(stats[1]["median_us"] / stats[0]["median_us"], 3)
            if "launches" not in out and beams > 1:
                out["launches"] = {k: library_launches(fn) for k, fn in zip(kinds, fns)}
        out["cells"].append(cell)
        del engines, fns
    print(json.dumps(out))


def sample_cells(args):
    """--sample: one msr3d_decode_sample launch beside one msr3d_decode_select launch on the same logits (8 previous
    tokens, repetition penalty 3), and a decode step followed by either, at the two shapes decoding has: 64 rows drawing
    one token (sampling without beams) and 5 prompts x 5 beams drawing 2 x beams candidates (beam sampling)."""
    net = build(args.layers)
    emb = torch.randn(VOCAB, HIDDEN, device="cuda").to(torch.bfloat16) * 0.02
    gen = torch.Generator(device="cuda").manual_seed(2)
    out = {"bench": "generate_sample", "device": torch.cuda.get_device_name(0), "layers": args.layers, "vocab": VOCAB,
           "repeats": args.repeats, "cells": []}
    for rows, k, order in ((64, 1, 0), (25, 10, 1)):
        lg = (torch.randn(rows, VOCAB, generator=gen, device="cuda") * 3.0).to(torch.bfloat16)
        prev = torch.randint(0, VOCAB, (rows, 8), generator=gen, device="cuda")
        bs = torch.zeros(rows, device="cuda") if order else None
        x = (torch.randn(1, 320, HIDDEN, generator=gen, device="cuda") * 0.5).to(torch.bfloat16)
        eng = CachedDecoder(net)
        eng.reserve(rows, 2 * args.repeats + 16)
        eng.prefill(x, torch.ones(1, 320, dtype=torch.int64, device="cuda"))
        eng.expand(rows)
        tok = emb[torch.randint(0, VOCAB, (rows,), generator=gen, device="cuda")]
        select = lambda: eng.select(lg, prev, 3.0, 1, 2, bs, order, k)                                    # noqa: E731
        cell = {"rows": rows, "k": k, "order": order, "select": timed(select, args.repeats), "sample": {}}
        for name, (temperature, top_k, top_p) in {"top_k50_top_p0.9": (1.0, 50, 0.9), "top_p0.9": (0.7, 0, 0.9),
                                                  "top_k50": (1.0, 50, 1.0), "no_warper": (1.0, 0, 1.0)}.items():
            draw = lambda: eng.sample(lg, prev, 3.0, 1, 2, bs, order, temperature, top_k, top_p, 1 + order, k, 1, 0, 0)  # noqa: E731,B023
            cell["sample"][name] = timed(draw, args.repeats)
        cell["step_then_select"] = timed(lambda: (eng.step(tok), select()), args.repeats)
        cell["step_then_sample"] = timed(lambda: (eng.step(tok), eng.sample(lg, prev, 3.0, 1, 2, bs, order, 1.0, 50, 0.9,
                                                                            1 + order, k, 1, 0, 0)), args.repeats)
        out["cells"].append(cell)
        del eng
    print(json.dumps(out))


def loop_cells(args):
    """--loop: whole tokens of `search` -- select, the beam bookkeeping, the step with its reorder -- under loop="host"
    (the parent's loop: torch bookkeeping, one synchronisation a token) and loop="device" (graph replays, the advance
    kernels, `done` read every `poll` tokens), alternating call by call in one process.  A cell's rows are whole prompts
    of 5 beams, repetition_penalty 3.0 (1 row: greedy search, no reorder).  eos_id=None, so a call runs exactly
    max_length tokens.  Host clock around whole `search` calls that end in a synchronise (the result is read); a token is
    (T(SHORT + RUN tokens) - T(SHORT tokens)) / RUN: both calls hold the same prefill, eager first token and captures, the
    difference is RUN steady-state tokens.  The capture's cost: the engine's own record (CachedDecoder.capture_seconds)."""
    from msr3d_amd.llm.generate import _embed_fn, search
    SHORT, RUN = 8, 32
    loops = ["host", "device"] if args.loop == "both" else [args.loop]
    polls = [int(p) for p in args.polls.split(",")]
    emb = torch.randn(VOCAB, HIDDEN, device="cuda").to(torch.bfloat16) * 0.02
    embed = _embed_fn(emb)
    gen = torch.Generator(device="cuda").manual_seed(1)
    captured = []                                                 # host seconds of every graph capture (the engine's record)

    def call(net, x, mask, beams, loop, tokens, poll):
        kw = dict(loop="device", poll=poll) if loop == "device" else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng = CachedDecoder(net)
        out = search(eng, embed, x, mask, eos_id=None, num_beams=beams, max_length=tokens, min_length=1,
                     repetition_penalty=3.0, **kw)
        out.cpu()
        captured.extend(eng.capture_seconds)
        return time.perf_counter() - t0

    def cell(net, layers, rows, length, sweep):
        beams = 1 if rows < BEAMS else BEAMS
        prompts = max(1, rows // beams)
        x = (torch.randn(prompts, length, HIDDEN, generator=gen, device="cuda") * 0.5).to(torch.bfloat16)
        mask = torch.ones(prompts, length, dtype=torch.int64, device="cuda")
        variants = [(lp, args.poll) for lp in loops] + ([("device", p) for p in polls if p != args.poll] if sweep else [])
        ts = {v: ([], []) for v in variants}
        del captured[:]
        for rep in range(args.repeats + 1):                       # (the first repeat is the warm-up)
            for v in variants:
                a, b = call(net, x, mask, beams, v[0], SHORT, v[1]), call(net, x, mask, beams, v[0], SHORT + RUN, v[1])
                if rep:
                    ts[v][0].append(a)
                    ts[v][1].append(b)
        c = {"layers": layers, "live_rows": prompts * beams, "prompts": prompts, "beams": beams, "length": length,
             "floor_us": round(step_bytes(layers, prompts * beams, length + SHORT + RUN // 2) / COPY_RATE * 1e6, 1)}
        for v in variants:
            per = sorted((b - a) / RUN * 1e6 for a, b in zip(*ts[v]))
            key = v[0] if v[1] == args.poll or v[0] == "host" else f"device_poll{v[1]}"
            c[key] = {"token_us": _stats(per), "call_short_ms": round(statistics.median(ts[v][0]) * 1e3, 2)}
        if captured:
            c["capture_ms_per_graph"] = round(statistics.median(captured) * 1e3, 2)
            c["graphs_per_group"] = 2 if beams > 1 else 1
        if "host" in c and "device" in c:
            c["device_over_host"] = round(c["device"]["token_us"]["median_us"] / c["host"]["token_us"]["median_us"], 3)
        return c

    out = {"bench": "generate_loop", "device": torch.cuda.get_device_name(0), "hidden": HIDDEN, "heads": HEADS, "vocab": VOCAB,
           "repeats": args.repeats, "tokens_timed": RUN, "poll": args.poll, "polls_swept": polls, "loops": loops, "cells": []}
    rows_arg = args.rows or "1,5,20,60"
    sweep_at = {(5, 320), (20, 320), (60, 576)}
    if args.layers:
        net = build(args.layers)
        for rows in (int(r) for r in rows_arg.split(",")):
            for length in (int(t) for t in args.lengths.split(",")):
                out["cells"].append(cell(net, args.layers, rows, length, (rows, length) in sweep_at))
                print(json.dumps(out["cells"][-1]), file=sys.stderr, flush=True)
        del net
    if args.layers_once:
        torch.cuda.empty_cache()
        net = build(args.layers_once)
        out["cells"].append(cell(net, args.layers_once, 20, 320, True))
    print(json.dumps(out))


def step_launches(net, rows, length, gen, emb, steps=5):
    """Per-launch device time (the binding's census: events around EVERY library launch) of a split and of a fused step at
    `rows` x `length`, medians over layers and `steps` steps: the fused products by their place in the layer, and of the
    split step the same products, the norm in front of q | k | v and of gate | up, the final norm, and the append."""
    from msr3d_amd.llm.products import skinny_entry
    x = (torch.randn(1, length, HIDDEN, generator=gen, device="cuda") * 0.5).to(torch.bfloat16)
    mask = torch.ones(1, length, dtype=torch.int64, device="cuda")
    tok = emb[torch.randint(0, VOCAB, (rows,), generator=gen, device="cuda")]
    layers = len(net.layers)
    out = {}
    for form in ("split", "fused"):
        eng = CachedDecoder(net, lora="merged", step=form)
        eng.reserve(rows, steps + 8)
        eng.prefill(x, mask)
        eng.expand(rows)
        for _ in range(3):
            eng.step(tok)
        sink = {}
        _lib.set_timing_sink(sink, census=True)
        try:
            for _ in range(steps):
                eng.step(tok)
            torch.cuda.synchronize()
        finally:
            _lib.set_timing_sink(None)
        us = {k: [e0.elapsed_time(e1) * 1e3 for e0, e1 in v] for k, v in sink.items()}
        med = lambda t: round(statistics.median(t), 1)                       # noqa: E731

        def by_place(ts, per_layer, names):
            """a launch list in step order, `per_layer` a layer and one more at the step's end -> medians by place."""
            per_step = per_layer * layers + 1
            assert len(ts) == per_step * steps, (len(ts), per_step, steps)
            cols = [[] for _ in names]
            for i, t in enumerate(ts):
                j = i % per_step
                cols[per_layer if j == per_step - 1 else j % per_layer].append(t)
            return {n: med(c) for n, c in zip(names, cols)}
        if form == "fused" and "msr3d_bf16_skinny_fused" in us:
            out[form] = by_place(us["msr3d_bf16_skinny_fused"], 4, ("q|k|v", "o", "gate|up", "down", "head"))
        else:
            out[form] = {**by_place(us[skinny_entry(rows)], 4, ("q|k|v", "o", "gate|up", "down", "head")),
                         **{"norm_" + k: v for k, v in by_place(us["msr3d_rmsnorm_fwd"], 2, ("in", "post", "final")).items()},
                         "append": med(us["msr3d_rope_kv_append"])}
        out[form]["attention"] = med(us["msr3d_attn_decode"])
        del eng
    return out


def step_cells(args):
    """--step: whole tokens of `search` on merged weights under step="split" (the parent's step) and step="fused",
    alternating call by call in one process, under --loop host (default), device or both -- loop_cells' clock: host time
    around whole `search` calls that end in a synchronise, a token = (T(SHORT + RUN tokens) - T(SHORT tokens)) / RUN.
    Rows are whole prompts of 5 beams (1 row: greedy).  Beside every cell the streaming floor; per row count the
    per-launch times of the fused products and of the split launches they replace (step_launches)."""
    from msr3d_amd.llm.generate import _embed_fn, search
    from msr3d_amd.llm.products import FUSED_MAX_ROWS
    SHORT, RUN = 8, 32
    forms = ["split", "fused"] if args.step == "both" else [args.step]
    loops = ["host", "device"] if args.loop == "both" else [args.loop or "host"]
    emb = torch.randn(VOCAB, HIDDEN, device="cuda").to(torch.bfloat16) * 0.02
    embed = _embed_fn(emb)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def call(net, x, mask, beams, loop, form, tokens):
        kw = dict(loop="device", poll=args.poll) if loop == "device" else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = search(CachedDecoder(net, lora="merged", step=form), embed, x, mask, eos_id=None, num_beams=beams,
                     max_length=tokens, min_length=1, repetition_penalty=3.0, **kw)
        out.cpu()
        return time.perf_counter() - t0

    def cell(net, layers, rows, length):
        beams = 1 if rows < BEAMS else BEAMS
        prompts = max(1, rows // beams)
        x = (torch.randn(prompts, length, HIDDEN, generator=gen, device="cuda") * 0.5).to(torch.bfloat16)
        mask = torch.ones(prompts, length, dtype=torch.int64, device="cuda")
        variants = [(lp, f) for lp in loops for f in forms]
        ts = {v: ([], []) for v in variants}
        for r in range(args.repeats + 1):                         # (the first repeat is the warm-up)
            for v in variants:
                a, b = call(net, x, mask, beams, *v, SHORT), call(net, x, mask, beams, *v, SHORT + RUN)
                if r:
                    ts[v][0].append(a)
                    ts[v][1].append(b)
        c = {"layers": layers, "live_rows": prompts * beams, "prompts": prompts, "beams": beams, "length": length,
             "runs_fused_launches": prompts * beams <= FUSED_MAX_ROWS,
             "floor_us": round(step_bytes(layers, prompts * beams, length + SHORT + RUN // 2) / COPY_RATE * 1e6, 1)}
        for lp in loops:
            c[lp] = {f: _stats(sorted((b - a) / RUN * 1e6 for a, b in zip(*ts[(lp, f)]))) for f in forms}
            if len(forms) == 2:
                sp, fu = c[lp]["split"], c[lp]["fused"]
                c[lp]["fused_over_split"] = round(fu["median_us"] / sp["median_us"], 3)
                # by spread: slower when fused's minimum lies above split's maximum, faster the other way round
                c[lp]["verdict"] = ("slower" if fu["min_us"] > sp["max_us"] else
                                    "faster" if fu["max_us"] < sp["min_us"] else "within the spread")
        return c

    out = {"bench": "generate_step", "device": torch.cuda.get_device_name(0), "hidden": HIDDEN, "heads": HEADS, "vocab": VOCAB,
           "repeats": args.repeats, "tokens_timed": RUN, "poll": args.poll, "loops": loops, "forms": forms,
           "fused_max_rows": FUSED_MAX_ROWS, "cells": [], "launches_us": {}}
    if args.layers:
        net = build(args.layers)
        net.merged_weights()
        for rows in (int(r) for r in (args.rows or "1,5,20,60").split(",")):
            for length in (int(t) for t in args.lengths.split(",")):
                out["cells"].append(cell(net, args.layers, rows, length))
                print(json.dumps(out["cells"][-1]), file=sys.stderr, flush=True)
            if len(forms) == 2:
                out["launches_us"][str(rows)] = step_launches(net, rows, 320, gen, emb)
                print(json.dumps({"launches_us": {rows: out["launches_us"][str(rows)]}}), file=sys.stderr, flush=True)
        del net
    if args.layers_once:
        torch.cuda.empty_cache()
        net = build(args.layers_once)
        net.merged_weights()
        out["cells"].append(cell(net, args.layers_once, 20, 320))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", action="store_true", help="time the draw kernel beside the select kernel and a step")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rows", default=None, help="live rows, comma-separated (default: the mode's own grid)")
    ap.add_argument("--lengths", default="128,320,576")
    ap.add_argument("--profile", default="", help="ROWSxLENGTH: only run that decode step 20 times (for a kernel trace)")
    ap.add_argument("--lora", default="separate", choices=("separate", "merged", "both"),
                    help="the engine's products; both: the two steps timed in turn in one process")
    ap.add_argument("--prompt-cache", default="", choices=("", "rows", "shared", "both"),
                    help="time a beam step (5 rows a prompt, a reorder in it) under that cache layout; both: in turn")
    ap.add_argument("--weights", default="", choices=("", "bf16", "e4m3", "both"),
                    help="time the step on those weights (e4m3: a base='fp8' stack); both: the two stacks in turn")
    ap.add_argument("--kv", default="", choices=("", "bf16", "e4m3", "both"),
                    help="time the step on that key / value cache (with --prompt-cache rows|shared, --lora separate|merged); "
                         "both: the two caches in turn, and the attention, append and reorder launches of each")
    ap.add_argument("--loop", default="", choices=("", "host", "device", "both"),
                    help="time whole tokens of search under that token loop; both: the two loops in turn")
    ap.add_argument("--step", default="", choices=("", "split", "fused", "both"),
                    help="time whole tokens of search on merged weights (--lora merged) under that step form, with --loop "
                         "host|device|both; both: the two forms in turn, and the fused products' launches beside the split ones")
    ap.add_argument("--poll", type=int, default=4, help="--loop: tokens between two reads of `done`")
    ap.add_argument("--polls", default="1,4,8,16", help="--loop: the values of poll swept at three cells")
    ap.add_argument("--layers-once", type=int, default=0, help="--loop: one more cell (20 x 320) on a stack this deep")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_generate needs a GPU"
    if args.step:
        if args.lora != "merged":
            ap.error("--step needs --lora merged (step='fused' runs on the merged planes)")
        return step_cells(args)
    if args.loop:
        return loop_cells(args)
    if args.sample:
        return sample_cells(args)
    if args.kv:
        return kv_cells(args)
    if args.weights:
        return weights_cells(args)
    if args.prompt_cache:
        return prompt_cache_cells(args)
    net = build(args.layers)
    emb = torch.randn(VOCAB, HIDDEN, device="cuda").to(torch.bfloat16) * 0.02
    gen = torch.Generator(device="cuda").manual_seed(1)
    grid = [(int(r), int(t)) for r in (args.rows or "1,5,20,32,40,64").split(",") for t in args.lengths.split(",")]
    if args.profile:
        grid = [tuple(int(v) for v in args.profile.split("x"))]
    out = {"bench": "generate", "device": torch.cuda.get_device_name(0), "layers": args.layers, "hidden": HIDDEN,
           "heads": HEADS, "inter": INTER, "vocab": VOCAB, "repeats": args.repeats, "copy_rate_TBps": COPY_RATE / 1e12,
           "lora": args.lora, "cells": []}
    if args.lora != "separate" and not args.profile:
        out["merge"] = merge_cell(net, args.repeats)
    for rows, length in grid:
        x = (torch.randn(1, length, HIDDEN, generator=gen, device="cuda") * 0.5).to(torch.bfloat16)
        mask = torch.ones(1, length, dtype=torch.int64, device="cuda")
        eng = CachedDecoder(net, lora="merged" if args.lora == "merged" else "separate")
        eng.reserve(rows, args.repeats + 8)
        prefill = None
        if not args.profile:
            prefill = timed(lambda: eng.prefill(x, mask), max(5, args.repeats // 4), warmup=2)
        eng.prefill(x, mask)
        eng.expand(rows)
        tok = emb[torch.randint(0, VOCAB, (rows,), generator=gen, device="cuda")]
        if args.lora == "both":
            other = CachedDecoder(net, lora="merged")
            other.reserve(rows, args.repeats + 8)
            other.prefill(x, mask)
            other.expand(rows)
            cached, merged = timed_alternating([lambda: eng.step(tok), lambda: other.step(tok)], args.repeats)
        else:
            cached, merged = timed(lambda: eng.step(tok), args.repeats), None
        cell = {"rows": rows, "length": length, "prefill_1row": prefill, "step": cached}
        if merged is not None:
            cell["step_merged"] = merged
            cell["merged_over_separate"] = round(merged["median_us"] / cached["median_us"], 3)
            if "launches" not in out:
                a, b = library_launches(lambda: eng.step(tok)), library_launches(lambda: other.step(tok))
                out["launches"] = {"separate": sum(a.values()), "merged": sum(b.values()), "separate_by_entry": a,
                                   "merged_by_entry": b, "torch_ops_per_step": 2}
            del other
        floor = step_bytes(args.layers, rows, length) / COPY_RATE * 1e6
        cell["floor_us"] = round(floor, 1)
        cell["floor_fraction"] = round(floor / cached["median_us"], 3)
        if not args.profile:
            # the parent's way: a full forward over the 64-padded prefix (length + 1 tokens), logits of the last one only
            Tp = -(-(length + 1) // 64) * 64
            xf = (torch.randn(rows, Tp, HIDDEN, generator=gen, device="cuda") * 0.5).to(torch.bfloat16)
            mf = torch.ones(rows, Tp, dtype=torch.uint8, device="cuda")
            mf[:, length + 1:] = 0
            with torch.no_grad():
                full = timed(lambda: net.logits(xf, mf, from_position=length), max(5, args.repeats // 2), warmup=2)
            cell["full_forward"] = full
            cell["speedup"] = round(full["median_us"] / cached["median_us"], 2)
        out["cells"].append(cell)
        del eng
    print(json.dumps(out))


if __name__ == "__main__":
    main()
