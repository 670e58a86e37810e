"""`KVCache`: the key / value buffers of one decoding call and everything that depends on their layout, which the engine
(generate.CachedDecoder) chooses once, when it allocates."""
import ctypes

import torch

from .._lib import call, current_stream_ptr, load, ptr


# ---- kv="e4m3": the cache format, stated once -------------------------------------------------------------------------
# Per (slot, head), over the head_dim values of K (rotated and rounded to bf16: what the bf16 cache stores) and,
# separately, of V: one power-of-two scale 2^e, e the smallest integer with amax 2^-e <= 448 (the largest e4m3), kept as
# one biased byte (e8m0: 2^(b - 127)), and OCP e4m3 codes of x 2^-e.  The scaling is exact and nothing saturates, so a
# code is ONE rounding of x, and code 2^e is a bf16 number: an e4m3 cache IS a bf16 cache whose every write went through
# dequantize(quantize(.)), which is how KVCache(dtype="e4m3", kernels=False) states it and what the kernels are tested
# against bit for bit.  e is clamped at -126 (b >= 1) so that 2^e and 2^-e are normal fp32 numbers: a head whose amax is
# below 2^-118 keeps e = -126 and its values round towards 0 like any value far below its head's amax.
def torch_kv_quantize(x):
    """x (..., heads, head_dim), any float dtype, any device -> codes (..., heads, head_dim) uint8 (e4m3 bit patterns),
    exps (..., heads) uint8 (biased exponents)."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    m, ex = torch.frexp(amax)                                  # amax = m 2^ex, m in [0.5, 1): 448 = 0.875 2^9
    e = torch.where(m <= 0.875, ex - 9, ex - 8).clamp_min(-126)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    codes = torch.ldexp(xf, -e[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, (e + 127).to(torch.uint8)


def torch_kv_dequantize(codes, exps):
    """-> (..., heads, head_dim) bf16 = code 2^(b - 127), exactly."""
    return torch.ldexp(codes.view(torch.float8_e4m3fn).float(), exps.to(torch.int32)[..., None] - 127).bfloat16()


def _kv_round(x):
    return torch_kv_dequantize(*torch_kv_quantize(x))


class KVCache:
    """layout "rows": kv[side] (layers, 2, rows, t_max, heads, head_dim) bf16, token-major like the projections' own
    output, side = `cur` is the live one (two sides only with `pingpong`: msr3d_kv_reorder gathers from one into the
    other); len (cache slots in use), pos (the next rotary position = number of unmasked tokens so far) (rows) int32; keep
    (key padding) (rows, t_max) uint8.  Allocated once per call, never resized.

    layout "shared" (`prompts` prompts of rows / prompts adjacent rows each, `t_prompt` prompt slots): a prompt's keys
    are written once by the prefill and are the same in all of its rows for ever, so they are stored once --
    prompt_kv (layers, 2, prompts, t_prompt, heads, head_dim), one side, never reordered, with prompt_keep (prompts,
    t_prompt) -- and only the generated tail is per row: kv[side] (layers, 2, rows, t_max - t_prompt, heads, head_dim),
    ping-ponged like the rows layout's.  `len` (rows) counts TAIL slots (what msr3d_rope_kv_append and msr3d_kv_reorder
    read on the tail planes) and `tail_len` (prompts) is the same number per prompt (what msr3d_attn_decode_shared
    reads): all rows of a prompt have the same length at every step, and a reorder permutes rows within a prompt, so
    neither is reordered.  `pos` is as in the rows layout.

    dtype "e4m3" (torch_kv_quantize above states the format): every plane above holds uint8 codes in the same shape, and
    beside each a plane of exponents, one byte per (slot, head) in slot records padded to 16 bytes -- kve[side] (layers,
    2, rows, slots, ceil16(heads)) and prompt_kve -- so that msr3d_kv_reorder, which moves 16-byte pieces, gathers them
    with a second call; they follow the codes through write_prompt, expand, reorder and flip.  With `kernels=False` the
    planes stay bf16 on the bf16 kernels and every write is rounded through the format in torch: THE statement of
    kv="e4m3", which the e4m3 kernels equal bit for bit."""

    def __init__(self, layers, rows, t_max, heads, head_dim, device, pingpong=False, layout="rows", prompts=None,
                 t_prompt=None, dtype="bf16", kernels=True):
        if layout not in ("rows", "shared"):
            raise ValueError(f"KVCache: layout is 'rows' or 'shared', not {layout!r}")
        if dtype not in ("bf16", "e4m3"):
            raise ValueError(f"KVCache: dtype is 'bf16' or 'e4m3', not {dtype!r}")
        self.layers, self.rows, self.t_max, self.heads, self.head_dim = layers, rows, t_max, heads, head_dim
        self.layout, self.shared = layout, layout == "shared"
        self.dtype = dtype
        self.codes = dtype == "e4m3" and bool(kernels)        # uint8 planes + exponents, read by the e4m3 kernels
        self.rounds = dtype == "e4m3" and not kernels         # bf16 planes, every write rounded in torch
        self.exp_pad = -(-heads // 16) * 16
        sides = 2 if pingpong else 1
        bf = torch.uint8 if self.codes else torch.bfloat16
        exps = lambda n, t, k=1: ([torch.zeros((layers, 2, n, t, self.exp_pad), dtype=torch.uint8, device=device)  # noqa: E731
                                   for _ in range(k)] if self.codes else None)
        mk = lambda *s, dt: [torch.zeros(s, dtype=dt, device=device) for _ in range(sides)]     # noqa: E731
        self._pos = mk(rows, dt=torch.int32)
        if not self.shared:
            self.kv = [torch.zeros((layers, 2, rows, t_max, heads, head_dim), dtype=bf, device=device) for _ in range(sides)]
            self._len = mk(rows, dt=torch.int32)
            self.kve = exps(rows, t_max, sides)
            self._keep = [torch.ones((rows, t_max), dtype=torch.uint8, device=device) for _ in range(sides)]
        else:
            if not prompts or rows % prompts or not t_prompt or not 0 < t_prompt < t_max:
                raise ValueError("KVCache: layout='shared' takes prompts (a divisor of rows) and 0 < t_prompt < t_max")
            self.prompts, self.t_prompt, self.t_tail = int(prompts), int(t_prompt), int(t_max - t_prompt)
            self.prompt_kv = torch.zeros((layers, 2, prompts, t_prompt, heads, head_dim), dtype=bf, device=device)
            self.prompt_keep = torch.ones((prompts, t_prompt), dtype=torch.uint8, device=device)
            self.kv = [torch.zeros((layers, 2, rows, self.t_tail, heads, head_dim), dtype=bf, device=device)
                       for _ in range(sides)]
            self.kve = exps(rows, self.t_tail, sides)
            self.prompt_kve = exps(prompts, t_prompt)[0] if self.codes else None
            # one buffer, so that one add_ advances both views: [rows tail lengths | prompts tail lengths]
            self._lens = torch.zeros(rows + prompts, dtype=torch.int32, device=device)
        if self.codes:
            # the per-layer (K, V) exponent views a step passes, made once: a step is host-bound at few rows
            self._exps = [[(t[i, 0], t[i, 1]) for i in range(layers)] for t in self.kve]
            self._prompt_exps = [(self.prompt_kve[i, 0], self.prompt_kve[i, 1]) for i in range(layers)] if self.shared else None
        self.cur = 0
        splits = load().msr3d_attn_decode_splits(rows, heads)
        self.workspace = (torch.empty(rows * heads * splits * (head_dim + 2), dtype=torch.float32, device=device)
                          if splits > 1 else None)

    len = property(lambda self: self._lens[:self.rows] if self.shared else self._len[self.cur])
    pos = property(lambda self: self._pos[self.cur])
    keep = property(lambda self: self._keep[self.cur])
    tail_len = property(lambda self: self._lens[self.rows:])

    @property
    def nbytes(self):
        """The bytes of the K / V planes allocated (every side, the prompt planes of the shared layout, and under e4m3 the
        exponent planes); the lengths, positions, key padding and the split workspace beside them are KB."""
        planes = list(self.kv) + ([self.prompt_kv] if self.shared else [])
        if self.codes:
            planes += list(self.kve) + ([self.prompt_kve] if self.shared else [])
        return sum(t.numel() * t.element_size() for t in planes)

    def k(self, layer):
        return self.kv[self.cur][layer, 0]

    def v(self, layer):
        return self.kv[self.cur][layer, 1]

    # -- the prefill: one row per prompt is written (a prompt's first); expand() fills the others -----------------------
    def _quantize(self, x):
        """msr3d_kv_quantize_e4m3 on x (prompts, T, heads, head_dim) bf16 -> codes, the same shape, and exps (prompts,
        T, exp_pad)."""
        x = x.contiguous()
        P, T, H, D = x.shape
        codes = torch.empty((P, T, H, D), dtype=torch.uint8, device=x.device)
        exps = torch.zeros((P, T, self.exp_pad), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            call("msr3d_kv_quantize_e4m3", P * T, H, D, ptr(x), H * D, ptr(codes), ptr(exps), self.exp_pad,
                 current_stream_ptr(x.device))
        return codes, exps

    def write_prompt(self, layer, k, v):
        """k, v (prompts, T, heads, head_dim) of a layer.  Shared: the one copy every row of the prompt reads.  e4m3:
        what is STORED is rounded; the prefill's own attention reads the k, v it was given."""
        first, T = slice(0, self.rows, self.rows // k.shape[0]), k.shape[1]
        for side, x in enumerate((k, v)):
            if self.codes:
                x, e = self._quantize(x)
                if self.shared:
                    self.prompt_kve[layer, side] = e
                else:
                    self.kve[self.cur][layer, side][first, :T] = e
            elif self.rounds:
                x = _kv_round(x)
            if self.shared:
                self.prompt_kv[layer, side] = x
            else:
                self.kv[self.cur][layer, side][first, :T] = x

    def close_prompt(self, pos, keep):
        """pos (prompts,) or a number: the next rotary position; keep (prompts, T) uint8: the prompt's key padding.
        (Shared: the tails are empty, len and tail_len stay 0.)"""
        first, T = slice(0, self.rows, self.rows // keep.shape[0]), keep.shape[1]
        self.pos[first] = pos
        if self.shared:
            self.prompt_keep.copy_(keep)
        else:
            self.len[first] = T
            self.keep[first, :T] = keep

    def expand(self, beams, T):
        """Every prompt's first row into its `beams` - 1 others: K / V of the T prompt slots and len, pos, keep.  Shared:
        pos alone -- no K / V to copy, the prompt planes serve every row."""
        B = self.rows // beams
        if self.shared:
            per_row = (self.pos,)
        else:
            for planes in (self.kv, self.kve) if self.codes else (self.kv,):
                p = planes[self.cur]
                kv = p.view(self.layers, 2, B, beams, self.t_max, *p.shape[4:])
                kv[:, :, :, 1:, :T] = kv[:, :, :, :1, :T]
            per_row = (self.len, self.pos, self.keep)
        for t in per_row:
            g = t.view(B, beams, *t.shape[1:])
            g[:, 1:] = g[:, :1]

    def attend(self, layer, q, k, v, cos, sin, table_rows, scale):
        """q, k, v (rows, heads head_dim) of the new token -> context, the same shape: q and k rotated by `pos` and k, v
        appended at slot `len` (shared: of the tail planes), then the decode attention over the cache (shared: the prompt
        planes once per prompt, then the tails; splits 0 = what the rows layout takes).  e4m3: the same two launches on
        the codes and exponents; as the statement (kernels=False), the bf16 launches with the appended slot rounded in
        between -- gathered and scattered by the device `len`, no synchronisation."""
        N, H, D = self.rows, self.heads, self.head_dim
        HD = H * D
        ck, cv = self.k(layer), self.v(layer)
        if self.codes:
            ctx = torch.empty((N, HD), dtype=torch.bfloat16, device=q.device)
            return self._attend_codes(layer, q, k, v, cos, sin, table_rows, scale, ctx)
        with torch.cuda.device(q.device):
            call("msr3d_rope_kv_append", N, H, D, ck.shape[1], ptr(q), ptr(k), ptr(v), HD, ptr(self.pos), ptr(self.len),
                 ptr(cos), ptr(sin), table_rows, ptr(ck), ptr(cv), current_stream_ptr(q.device))
            if self.rounds:
                # (a full cache: nothing was appended and the last slot, rounded already, is rounded again: unchanged)
                rows = torch.arange(N, device=q.device)
                slot = self.len.long().clamp(0, ck.shape[1] - 1)
                ck[rows, slot] = _kv_round(ck[rows, slot])
                cv[rows, slot] = _kv_round(cv[rows, slot])
        return self.attend_appended(layer, q, scale)

    def planes(self, layer):
        """-> (k plane, v plane, slots a row) of `layer` as a step appends to them: what msr3d_rope_kv_append is given
        (shared: the tail planes).  For a product that does the append itself (step="fused", the plain bf16 cache)."""
        ck = self.k(layer)
        return ck, self.v(layer), ck.shape[1]

    def attend_appended(self, layer, q, scale):
        """`attend` from its second launch on, for the bf16 planes: q (rows, heads head_dim) is rotated and slot `len`
        holds the new token's k, v already -> context."""
        if self.codes:
            raise RuntimeError("KVCache.attend_appended: the e4m3 cache appends through `attend` (its quantiser)")
        N, H, D = self.rows, self.heads, self.head_dim
        HD, ws = H * D, self.workspace
        ck, cv = self.k(layer), self.v(layer)
        ctx = torch.empty((N, HD), dtype=torch.bfloat16, device=q.device)
        with torch.cuda.device(q.device):
            s = current_stream_ptr(q.device)
            if self.shared:
                call("msr3d_attn_decode_shared", self.prompts, N // self.prompts, self.t_prompt, self.t_tail, H, D, ptr(q),
                     HD, ptr(self.prompt_kv[layer, 0]), ptr(self.prompt_kv[layer, 1]), ptr(self.prompt_keep), ptr(ck),
                     ptr(cv), ptr(self.tail_len), 1, ctypes.c_float(scale), ptr(ctx), HD, ptr(ws),
                     ws.numel() if ws is not None else 0, 0, s)
            else:
                call("msr3d_attn_decode", N, self.t_max, H, D, ptr(q), HD, ptr(ck), ptr(cv), ptr(self.len), 1,
                     ptr(self.keep), ctypes.c_float(scale), ptr(ctx), HD, ptr(ws), ws.numel() if ws is not None else 0, s)
        return ctx

    def _attend_codes(self, layer, q, k, v, cos, sin, table_rows, scale, ctx):
        N, H, D, E = self.rows, self.heads, self.head_dim, self.exp_pad
        HD, ws = H * D, self.workspace
        ck, cv = self.k(layer), self.v(layer)
        ek, ev = self._exps[self.cur][layer]
        with torch.cuda.device(q.device):
            s = current_stream_ptr(q.device)
            call("msr3d_rope_kv_append_e4m3", N, H, D, ck.shape[1], ptr(q), ptr(k), ptr(v), HD, ptr(self.pos),
                 ptr(self.len), ptr(cos), ptr(sin), table_rows, ptr(ck), ptr(cv), ptr(ek), ptr(ev), E, s)
            if self.shared:
                call("msr3d_attn_decode_shared_e4m3", self.prompts, N // self.prompts, self.t_prompt, self.t_tail, H, D,
                     ptr(q), HD, ptr(self.prompt_kv[layer, 0]), ptr(self.prompt_kv[layer, 1]),
                     ptr(self._prompt_exps[layer][0]), ptr(self._prompt_exps[layer][1]), ptr(self.prompt_keep), ptr(ck),
                     ptr(cv), ptr(ek), ptr(ev), E, ptr(self.tail_len), 1, ctypes.c_float(scale), ptr(ctx), HD, ptr(ws),
                     ws.numel() if ws is not None else 0, 0, s)
            else:
                call("msr3d_attn_decode_e4m3", N, self.t_max, H, D, ptr(q), HD, ptr(ck), ptr(cv), ptr(ek), ptr(ev), E,
                     ptr(self.len), 1, ptr(self.keep), ctypes.c_float(scale), ptr(ctx), HD, ptr(ws),
                     ws.numel() if ws is not None else 0, s)
        return ctx

    def advance(self):
        """One more slot in use and one more position, in every row."""
        (self._lens if self.shared else self._len[self.cur]).add_(1)
        self.pos.add_(1)

    def reorder(self, beam_idx):
        """Row n continues row beam_idx[n]: one launch for every layer's K and V, into the other side (e4m3: a second
        one for the exponent planes, whose slot records are whole 16-byte pieces).  Shared layout: the tail planes
        alone, and beam_idx[n] must be a row of n's own prompt (what beam search produces)."""
        if len(self.kv) < 2:
            raise RuntimeError("KVCache: allocated without the second side (pingpong=True) a reorder needs")
        idx = beam_idx.to(torch.int32).contiguous()
        src, dst = self.kv[self.cur], self.kv[1 - self.cur]
        dev = src.device
        with torch.cuda.device(dev):
            # (row_elems counts 2-byte elements)
            call("msr3d_kv_reorder", self.layers * 2, self.rows, src.shape[3],
                 self.heads * self.head_dim // (2 if self.codes else 1), ptr(src), ptr(dst), ptr(idx), ptr(self.len),
                 current_stream_ptr(dev))
            if self.codes:
                call("msr3d_kv_reorder", self.layers * 2, self.rows, src.shape[3], self.exp_pad // 2,
                     ptr(self.kve[self.cur]), ptr(self.kve[1 - self.cur]), ptr(idx), ptr(self.len), current_stream_ptr(dev))
        il = idx.long()
        for pair in ((self._pos,) if self.shared else (self._len, self._pos, self._keep)):
            torch.index_select(pair[self.cur], 0, il, out=pair[1 - self.cur])
        self.cur = 1 - self.cur

    def flip(self):
        """The other side becomes the live one.  For a captured token (CachedDecoder.token_loop): the capture of a
        `reorder` flips `cur` without moving a byte, so the loop flips it back, and flips it after every replay of a
        graph that holds a reorder -- `cur` then names the side the data is on, as after an eager reorder."""
        if len(self.kv) < 2:
            raise RuntimeError("KVCache: allocated without a second side")
        self.cur = 1 - self.cur
