"""`KVCache`: the key / value buffers of one decoding call and everything that depends on their layout, which the engine
(generate.CachedDecoder) chooses once, when it allocates."""
import ctypes

import torch

from .._lib import call, current_stream_ptr, load, ptr


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
    neither is reordered.  `pos` is as in the rows layout."""

    def __init__(self, layers, rows, t_max, heads, head_dim, device, pingpong=False, layout="rows", prompts=None,
                 t_prompt=None):
        if layout not in ("rows", "shared"):
            raise ValueError(f"KVCache: layout is 'rows' or 'shared', not {layout!r}")
        self.layers, self.rows, self.t_max, self.heads, self.head_dim = layers, rows, t_max, heads, head_dim
        self.layout, self.shared = layout, layout == "shared"
        sides = 2 if pingpong else 1
        bf = torch.bfloat16
        mk = lambda *s, dt: [torch.zeros(s, dtype=dt, device=device) for _ in range(sides)]     # noqa: E731
        self._pos = mk(rows, dt=torch.int32)
        if not self.shared:
            self.kv = [torch.zeros((layers, 2, rows, t_max, heads, head_dim), dtype=bf, device=device) for _ in range(sides)]
            self._len = mk(rows, dt=torch.int32)
            self._keep = [torch.ones((rows, t_max), dtype=torch.uint8, device=device) for _ in range(sides)]
        else:
            if not prompts or rows % prompts or not t_prompt or not 0 < t_prompt < t_max:
                raise ValueError("KVCache: layout='shared' takes prompts (a divisor of rows) and 0 < t_prompt < t_max")
            self.prompts, self.t_prompt, self.t_tail = int(prompts), int(t_prompt), int(t_max - t_prompt)
            self.prompt_kv = torch.zeros((layers, 2, prompts, t_prompt, heads, head_dim), dtype=bf, device=device)
            self.prompt_keep = torch.ones((prompts, t_prompt), dtype=torch.uint8, device=device)
            self.kv = [torch.zeros((layers, 2, rows, self.t_tail, heads, head_dim), dtype=bf, device=device)
                       for _ in range(sides)]
            # one buffer, so that one add_ advances both views: [rows tail lengths | prompts tail lengths]
            self._lens = torch.zeros(rows + prompts, dtype=torch.int32, device=device)
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
        """The bytes of the K / V planes allocated (every side, and the prompt planes of the shared layout); the lengths,
        positions, key padding and the split workspace beside them are KB."""
        n = sum(t.numel() * t.element_size() for t in self.kv)
        return n + (self.prompt_kv.numel() * self.prompt_kv.element_size() if self.shared else 0)

    def k(self, layer):
        return self.kv[self.cur][layer, 0]

    def v(self, layer):
        return self.kv[self.cur][layer, 1]

    # -- the prefill: one row per prompt is written (a prompt's first); expand() fills the others -----------------------
    def write_prompt(self, layer, k, v):
        """k, v (prompts, T, heads, head_dim) of a layer.  Shared: the one copy every row of the prompt reads."""
        if self.shared:
            self.prompt_kv[layer, 0] = k
            self.prompt_kv[layer, 1] = v
        else:
            first, T = slice(0, self.rows, self.rows // k.shape[0]), k.shape[1]
            self.k(layer)[first, :T] = k
            self.v(layer)[first, :T] = v

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
            kv = self.kv[self.cur].view(self.layers, 2, B, beams, self.t_max, self.heads, self.head_dim)
            kv[:, :, :, 1:, :T] = kv[:, :, :, :1, :T]
            per_row = (self.len, self.pos, self.keep)
        for t in per_row:
            g = t.view(B, beams, *t.shape[1:])
            g[:, 1:] = g[:, :1]

    def attend(self, layer, q, k, v, cos, sin, table_rows, scale):
        """q, k, v (rows, heads head_dim) of the new token -> context, the same shape: q and k rotated by `pos` and k, v
        appended at slot `len` (shared: of the tail planes), then the decode attention over the cache (shared: the prompt
        planes once per prompt, then the tails; splits 0 = what the rows layout takes)."""
        N, H, D = self.rows, self.heads, self.head_dim
        HD, ws = H * D, self.workspace
        ck, cv = self.k(layer), self.v(layer)
        ctx = torch.empty((N, HD), dtype=torch.bfloat16, device=q.device)
        with torch.cuda.device(q.device):
            s = current_stream_ptr(q.device)
            call("msr3d_rope_kv_append", N, H, D, ck.shape[1], ptr(q), ptr(k), ptr(v), HD, ptr(self.pos), ptr(self.len),
                 ptr(cos), ptr(sin), table_rows, ptr(ck), ptr(cv), s)
            if self.shared:
                call("msr3d_attn_decode_shared", self.prompts, N // self.prompts, self.t_prompt, self.t_tail, H, D, ptr(q),
                     HD, ptr(self.prompt_kv[layer, 0]), ptr(self.prompt_kv[layer, 1]), ptr(self.prompt_keep), ptr(ck),
                     ptr(cv), ptr(self.tail_len), 1, ctypes.c_float(scale), ptr(ctx), HD, ptr(ws),
                     ws.numel() if ws is not None else 0, 0, s)
            else:
                call("msr3d_attn_decode", N, self.t_max, H, D, ptr(q), HD, ptr(ck), ptr(cv), ptr(self.len), 1,
                     ptr(self.keep), ctypes.c_float(scale), ptr(ctx), HD, ptr(ws), ws.numel() if ws is not None else 0, s)
        return ctx

    def advance(self):
        """One more slot in use and one more position, in every row."""
        (self._lens if self.shared else self._len[self.cur]).add_(1)
        self.pos.add_(1)

    def reorder(self, beam_idx):
        """Row n continues row beam_idx[n]: one launch for every layer's K and V, into the other side.  Shared layout:
        the tail planes alone, and beam_idx[n] must be a row of n's own prompt (what beam search produces)."""
        if len(self.kv) < 2:
            raise RuntimeError("KVCache: allocated without the second side (pingpong=True) a reorder needs")
        idx = beam_idx.to(torch.int32).contiguous()
        src, dst = self.kv[self.cur], self.kv[1 - self.cur]
        dev = src.device
        with torch.cuda.device(dev):
            call("msr3d_kv_reorder", self.layers * 2, self.rows, src.shape[3], self.heads * self.head_dim, ptr(src), ptr(dst),
                 ptr(idx), ptr(self.len), current_stream_ptr(dev))
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
