"""Times the image-token hand-off (msr3d_amd/csrc/image_tokens.hip) at the reference's main configuration: B = 20 sequences,
N = 60 image slots each (msr3d_max_img_num), C = 1024 pooled ConvNeXt features, E = 4096 (Vicuna-7B), prompts of T tokens,
bf16 inputs_embeds; 0, 20, 200 and 1200 real images.

Per image count, in one process, ALTERNATING repeat by repeat:
  fused fwd   msr3d_image_project_scatter: map + compact + project + cast + scatter (2 launches), sized by B N, live count read
              on the device;
  dense fwd   the route a user of the pieces that were here before would write: hipops.module_linear over ALL B N slots, then
              the torch mirror's sync-free scatter (scatter_image_tokens);
  fused bwd   msr3d_image_project_grad (dW, db stored, placeholder rows cleared: 2 launches);
  dense bwd   autograd's backward of the dense route (the mirror's where / index_select backward + the HIP weight gradient
              over all B N rows), forward untimed.
Device events around every repeat (`inner` calls per window for the fused entries), warm-up first; median (min .. max) in us.
floor: the bytes the forward must move -- W once per 64-row band of live images, their features, their output rows -- at
6.29 TB/s (the rate a streaming copy reaches on an MI355X).  A record, not a gate.  Prints one JSON line; --table PATH writes
the table.

    python tools/bench_image_tokens.py [--repeats 9] [--T 640] [--table profiles/image_tokens.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from msr3d_amd import hipops  # noqa: E402
from msr3d_amd.model import image_tokens as it  # noqa: E402

B, N, C, E = 20, 60, 1024, 4096
COPY_RATE = 6.29e12
TOK = it.IMG_SP_TOKEN


def _stat(ts, inner=1):
    ts = sorted(t / inner for t in ts)
    return {"median_us": round(statistics.median(ts), 1), "min_us": round(ts[0], 1), "max_us": round(ts[-1], 1)}


def timed(fn, setup=None):
    if setup is not None:
        setup()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def cell(n_img, T, repeats, inner, gen):
    dev = torch.device("cuda")
    ids = torch.randint(3, 30000, (B, T), generator=gen)
    masks = torch.zeros(B, N, dtype=torch.bool)
    per_row = [n_img // B + (1 if b < n_img % B else 0) for b in range(B)]
    for b, k in enumerate(per_row):
        masks[b, :k] = True
        ids[b, torch.randperm(T, generator=gen)[:k]] = TOK
    ids, masks = ids.to(dev), masks.to(dev)
    fts = torch.randn(B, N, C, generator=gen).to(dev)
    lin = torch.nn.Linear(C, E).to(dev)
    emb = torch.randn(B, T, E, generator=gen).to(torch.bfloat16).to(dev)
    G = torch.randn(B, T, E, generator=gen).to(torch.bfloat16).to(dev)
    dW, db = torch.empty(E, C, device=dev), torch.empty(E, device=dev)
    state = {}

    def fused_fwd():
        with torch.no_grad():
            for _ in range(inner):
                state["map"] = it._launch(emb, None, ids, fts, masks, lin.weight, lin.bias, TOK, "interleaved")

    def dense_fwd():
        with torch.no_grad():
            for _ in range(inner):
                tok = hipops.module_linear(lin, fts)
                it.scatter_image_tokens(emb, None, ids, tok, masks, TOK, "interleaved")

    def fused_bwd():
        dest, src, cnt, f2 = state["map"]
        for _ in range(inner):
            it.image_project_grad(G, dest, src, cnt, f2, dW, db, accumulate=False, clear_rows=True)

    def dense_graph():
        lin.zero_grad(set_to_none=True)
        tok = hipops.module_linear(lin, fts)
        state["out"] = it.scatter_image_tokens(emb, None, ids, tok, masks, TOK, "interleaved")[0]

    def dense_bwd():
        state["out"].backward(G)

    fused_fwd()
    for fn in (fused_fwd, dense_fwd, fused_bwd):
        fn()
    dense_graph()
    dense_bwd()
    torch.cuda.synchronize()
    ts = {k: [] for k in ("fused_fwd", "dense_fwd", "fused_bwd", "dense_bwd")}
    for _ in range(repeats):
        ts["fused_fwd"].append(timed(fused_fwd))
        ts["dense_fwd"].append(timed(dense_fwd))
        ts["fused_bwd"].append(timed(fused_bwd))
        ts["dense_bwd"].append(timed(dense_bwd, setup=dense_graph))
    r = {"images": n_img, "fused_fwd": _stat(ts["fused_fwd"], inner), "dense_fwd": _stat(ts["dense_fwd"], inner),
         "fused_bwd": _stat(ts["fused_bwd"], inner), "dense_bwd": _stat(ts["dense_bwd"])}
    bands = -(-n_img // 64)
    r["fwd_floor_us"] = round((bands * E * C * 4 + n_img * C * 4 + n_img * E * 2) / COPY_RATE * 1e6, 2)
    r["fwd_ratio"] = round(r["dense_fwd"]["median_us"] / r["fused_fwd"]["median_us"], 2)
    r["bwd_ratio"] = round(r["dense_bwd"]["median_us"] / r["fused_bwd"]["median_us"], 2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--T", type=int, default=640)
    ap.add_argument("--images", default="0,20,200,1200")
    ap.add_argument("--table", default="")
    ap.add_argument("--commit", default="", help="the commit the tree stands on, for the table's header (default: ask git)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_image_tokens needs a GPU"
    gen = torch.Generator().manual_seed(1)
    out = {"bench": "image_tokens", "device": torch.cuda.get_device_name(0), "B": B, "N": N, "C": C, "E": E, "T": args.T,
           "repeats": args.repeats, "inner": args.inner, "copy_rate_TBps": COPY_RATE / 1e12,
           "cells": [cell(int(v), args.T, args.repeats, args.inner, gen) for v in args.images.split(",")]}
    print(json.dumps(out))
    if args.table:
        commit = args.commit
        try:
            commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                              cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip() or "unknown"
        except OSError:
            commit = commit or "unknown"
        f = lambda s: "%.1f (%.1f .. %.1f)" % (s["median_us"], s["min_us"], s["max_us"])       # noqa: E731
        lines = ["image tokens: fused project-and-scatter against the dense route, %s, B = %d, N = %d, C = %d, E = %d, T = %d, bf16 embeds"
                 % (out["device"], B, N, C, E, args.T),
                 "taken on the working tree on top of commit %s; device events, %d alternating repeats, median (min .. max), us per call"
                 % (commit, args.repeats),
                 "dense route: hipops.module_linear over all %d slots + the torch mirror's scatter; its backward through autograd" % (B * N),
                 "",
                 "%6s | %24s | %8s | %26s | %7s | %24s | %28s | %7s"
                 % ("images", "fused fwd (2 launches)", "floor", "dense fwd", "d / f", "fused bwd (2 launches)", "dense bwd", "d / f")]
        for c in out["cells"]:
            lines.append("%6d | %24s | %8.2f | %26s | %6.2fx | %24s | %28s | %6.2fx"
                         % (c["images"], f(c["fused_fwd"]), c["fwd_floor_us"], f(c["dense_fwd"]), c["fwd_ratio"], f(c["fused_bwd"]),
                            f(c["dense_bwd"]), c["bwd_ratio"]))
        os.makedirs(os.path.dirname(os.path.abspath(args.table)), exist_ok=True)
        with open(args.table, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
