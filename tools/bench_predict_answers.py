"""Times closed-set answer ranking (msr3d_amd/llm/generate.py::rank_answers' two engine calls) at Vicuna-7B layer shapes
with random weights: B = 4 prompts of T tokens, C candidates of S = 16 suffix tokens each.

Per cell (C, T), in one process, ALTERNATING repeat by repeat:
  shared   CachedDecoder.prefill(positions="arange") over the B prompts + CachedDecoder.score over the B C S suffix rows
           (attention: msr3d_attn_prefix_fwd against the one cached prefix);
  literal  what the reference does, on the full forward that was here before: LoRALlamaStack.logits over the B prompts
           (stage 1) and over the B C sequences of T + S tokens, padded to a multiple of 64 with masked rows (stage 3).
           Walked in chunks of --literal-chunk sequences (default 64: 512 sequences x 640 tokens x 4096 x 2 bytes is 2.7 GB
           per activation tensor), each with from_position = T - 1, so the last layer's MLP, the final norm and the head run
           over the answer span only -- the cheapest way the existing code offers, not the reference's whole-sequence head.
and the new kernel alone (one layer's launch: H = 32, D = 128) against
  floor    the bytes it must move -- the prefix K / V once per (prompt, head) + the suffix q, k, v, out -- at 6.29 TB/s (the
           rate a streaming copy reaches on an MI355X),
  order 1  the same launch with a (prompt, head)'s tiles numbered adjacently instead of 8 apart (msr3d_attn_prefix_order),
  attn_fwd msr3d_attn_fwd on the materialised repeated problem (B C sequences of ceil64(T + S) rows).
Device events around every repeat, warm-up first; median and min .. max.  Prints one JSON line and, with --table PATH,
writes the table.

    python tools/bench_predict_answers.py [--layers 4] [--repeats 7] [--cands 32,128] [--lengths 128,320,576] [--table PATH]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from msr3d_amd import _lib  # noqa: E402
from msr3d_amd.llm.generate import CachedDecoder  # noqa: E402
from tools.bench_generate import COPY_RATE, HEADS, HIDDEN, INTER, VOCAB, build  # noqa: E402

B, S, D = 4, 16, HIDDEN // HEADS


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stat(ts):
    ts = sorted(ts)
    return {"median_us": round(statistics.median(ts), 1), "min_us": round(ts[0], 1), "max_us": round(ts[-1], 1)}


def timed_alternating(fns, repeats, warmup=1):
    """fns: {name: callable}; every repeat runs each once, in turn -> {name: stats}."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n in fns}
    for _ in range(repeats):
        for n, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[n].append(e0.elapsed_time(e1) * 1e3)
    return {n: _stat(v) for n, v in ts.items()}


def kernel_cell(C, T, gen, repeats, inner=20):
    """One layer's attention launch, `inner` launches per timed window (-> us per launch)."""
    lib, dev = _lib.load(), torch.device("cuda")
    bf = lambda *s: torch.randn(*s, generator=gen, device="cuda").to(torch.bfloat16)     # noqa: E731
    HD = HEADS * D
    q, k, v = bf(B, C, S, HD), bf(B, C, S, HD), bf(B, C, S, HD)
    kc, vc = bf(B, T, HD), bf(B, T, HD)
    length = torch.full((B,), T, dtype=torch.int32, device="cuda")
    pkeep = torch.ones((B, T), dtype=torch.uint8, device="cuda")
    skeep = torch.ones((B * C, S), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(q)
    scale = ctypes.c_float(1.0 / math.sqrt(D))
    Tp = -(-(T + S) // 64) * 64
    qf, kf, vf = bf(B * C, Tp, HD), bf(B * C, Tp, HD), bf(B * C, Tp, HD)
    of = torch.empty_like(qf)
    keepf = torch.ones((B * C, Tp), dtype=torch.uint8, device="cuda")
    keepf[:, T + S:] = 0
    lse = torch.empty((B * C, HEADS, Tp), dtype=torch.float32, device="cuda")

    def prefix(order):
        def run():
            lib.msr3d_attn_prefix_order(order)
            st = _lib.current_stream_ptr(dev)
            for _ in range(inner):
                _lib.check(lib.msr3d_attn_prefix_fwd(B, C, S, T, HEADS, D, _p(q), _p(k), _p(v), HD, _p(kc), _p(vc), _p(length),
                                                     _p(pkeep), _p(skeep), scale, _p(out), HD, st), "msr3d_attn_prefix_fwd")
            lib.msr3d_attn_prefix_order(0)
        return run

    def materialised():
        st = _lib.current_stream_ptr(dev)
        for _ in range(inner):
            _lib.check(lib.msr3d_attn_fwd(B * C, Tp, HEADS, D, _p(qf), _p(kf), _p(vf), HD, _p(keepf), scale, _p(of), _p(lse), st),
                       "msr3d_attn_fwd")

    r = timed_alternating({"prefix": prefix(0), "prefix_order1": prefix(1), "attn_fwd_repeated": materialised}, repeats, warmup=2)
    for rec in r.values():
        for kk in rec:
            rec[kk] = round(rec[kk] / inner, 2)
    floor = (2 * B * T * HD * 2 + 4 * B * C * S * HD * 2) / COPY_RATE * 1e6
    r["floor_us"] = round(floor, 2)
    r["floor_fraction"] = round(floor / r["prefix"]["median_us"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cands", default="32,128")
    ap.add_argument("--lengths", default="128,320,576")
    ap.add_argument("--literal-chunk", type=int, default=64)
    ap.add_argument("--table", default="")
    ap.add_argument("--commit", default="", help="the commit the tree stands on, for the table's header (default: ask git)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_predict_answers needs a GPU"
    net = build(args.layers)
    gen = torch.Generator(device="cuda").manual_seed(1)
    out = {"bench": "predict_answers", "device": torch.cuda.get_device_name(0), "layers": args.layers, "hidden": HIDDEN,
           "heads": HEADS, "inter": INTER, "vocab": VOCAB, "B": B, "S": S, "repeats": args.repeats,
           "literal_chunk": args.literal_chunk, "copy_rate_TBps": COPY_RATE / 1e12, "cells": []}
    for C in [int(v) for v in args.cands.split(",")]:
        for T in [int(v) for v in args.lengths.split(",")]:
            x = (torch.randn(B, T, HIDDEN, generator=gen, device="cuda") * 0.5).to(torch.bfloat16)
            mask = torch.ones(B, T, dtype=torch.int64, device="cuda")
            suf = (torch.randn(B, C, S, HIDDEN, generator=gen, device="cuda") * 0.5).to(torch.bfloat16)
            sk = torch.ones(B, C, S, dtype=torch.bool, device="cuda")
            eng = CachedDecoder(net)
            eng.reserve(1, 0)

            def shared():
                eng.prefill(x, mask, positions="arange")
                return eng.score(suf, sk)

            Tp1, Tp3 = -(-T // 64) * 64, -(-(T + S) // 64) * 64
            x1 = torch.cat([x, torch.zeros((B, Tp1 - T, HIDDEN), dtype=x.dtype, device="cuda")], 1).contiguous()
            m1 = torch.cat([mask, torch.zeros((B, Tp1 - T), dtype=mask.dtype, device="cuda")], 1).to(torch.uint8).contiguous()
            n = min(args.literal_chunk, B * C)
            x3 = (torch.randn(n, Tp3, HIDDEN, generator=gen, device="cuda") * 0.5).to(torch.bfloat16)
            m3 = torch.ones(n, Tp3, dtype=torch.uint8, device="cuda")
            m3[:, T + S:] = 0

            def literal():
                with torch.no_grad():
                    net.logits(x1, m1, from_position=T - 1)
                    for _ in range(-(-B * C // n)):              # (every chunk has the same shapes: one buffer serves all)
                        net.logits(x3, m3, from_position=T - 1)

            def score_only():
                return eng.score(suf, sk)

            r = timed_alternating({"shared": shared, "literal": literal}, args.repeats, warmup=1)
            r.update(timed_alternating({"score_only": score_only}, args.repeats, warmup=1))
            cell = {"C": C, "T": T, **r, "speedup": round(r["literal"]["median_us"] / r["shared"]["median_us"], 2),
                    "tokens_literal": B * Tp1 + B * C * Tp3, "tokens_shared": B * Tp1 + B * C * S}
            cell["kernel"] = kernel_cell(C, T, gen, args.repeats)
            cell["kernel_share_of_score"] = round(args.layers * cell["kernel"]["prefix"]["median_us"] / r["score_only"]["median_us"], 4)
            out["cells"].append(cell)
            del eng
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.table:
        commit = args.commit
        try:
            commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                    cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip() or "unknown"
        except OSError:
            commit = commit or "unknown"
        lines = ["predict_answers: shared-prefix route against the literal route, %s, %d layers of Vicuna-7B shape, B = %d, S = %d"
                 % (out["device"], args.layers, B, S),
                 "taken on the working tree on top of commit %s; device events, %d alternating repeats, median (min .. max), us"
                 % (commit, args.repeats),
                 "literal route: chunks of %d sequences, from_position = T - 1" % args.literal_chunk, "",
                 "%4s %4s | %28s | %32s | %7s | %24s" % ("C", "T", "shared (prefill + score)", "literal (full forward)", "speedup",
                                                          "score alone"),
                 ]
        f = lambda s: "%.0f (%.0f .. %.0f)" % (s["median_us"], s["min_us"], s["max_us"])       # noqa: E731
        for c in out["cells"]:
            lines.append("%4d %4d | %28s | %32s | %6.2fx | %24s" % (c["C"], c["T"], f(c["shared"]), f(c["literal"]), c["speedup"],
                                                                     f(c["score_only"])))
        lines += ["", "msr3d_attn_prefix_fwd alone, one layer's launch (H = 32, D = 128), us per launch, median (min .. max)",
                  "%4s %4s | %22s | %8s | %8s | %22s | %22s | %14s" % ("C", "T", "prefix kernel", "floor", "floor/t", "tiles adjacent (order 1)",
                                                                        "attn_fwd, repeated", "share of score")]
        g = lambda s: "%.1f (%.1f .. %.1f)" % (s["median_us"], s["min_us"], s["max_us"])       # noqa: E731
        for c in out["cells"]:
            k = c["kernel"]
            lines.append("%4d %4d | %22s | %8.2f | %8.3f | %22s | %22s | %13.1f%%"
                         % (c["C"], c["T"], g(k["prefix"]), k["floor_us"], k["floor_fraction"], g(k["prefix_order1"]),
                            g(k["attn_fwd_repeated"]), 100 * c["kernel_share_of_score"]))
        os.makedirs(os.path.dirname(os.path.abspath(args.table)), exist_ok=True)
        with open(args.table, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
