"""How the decoding engine multiplies a layer's projections: decoder.ModuleProducts' operations (`project`, `gated`,
`head`) for the three weight sources of generate.CachedDecoder, each in two widths -- the source object itself is the WIDE
form (prefill and `score`: any number of token rows on the tiled GEMMs), its `.skinny` the form of one decode step (M <=
64 live rows: every product streams its weight once, members of one input group share the low-rank activation and ONE
launch, gate | up carry the SwiGLU epilogue; `skinny_project` is the one walk for all three).  No autograd in either.

    source                  wide                                      skinny: r-row launch -> operands          R
    SeparateProducts        the module call (ModuleProducts)          msr3d_bf16_gemm_skinny -> u               64
    MergedModuleProducts    one R = 0 GEMM on bf16(W + s B A)         none (P2 NULL)                            0
    E4m3Products            the module call from 128 rows up,         msr3d_bf16_gemm_skinny_quant -> u, the    64
                            64-row slabs on the skinny form below       e4m3 codes of h, their row scales"""
import ctypes

import torch

from .. import _lib
from .._lib import call, current_stream_ptr, ptr
from .decoder import ModuleProducts, _SwiGLUFn
from .lora import PAD_R, LoRALinear, _gemm, _skinny

E4M3_SLAB = 64          # MSR3D_SKINNY_WIDE_MAX_M: the rows one msr3d_fp8_skinny_lowrank launch takes
E4M3_WIDE_MIN = 128     # from here up LoRALinear's own forward multiplies on e4m3 (msr3d_fp8_gemm_lowrank's domain)


def skinny_entry(M):
    """The bf16 weight-stream product for M live rows: up to 32 the entry every call has used so far (the same bits), the
    wide one (three or four activation tiles) for 33 .. 64."""
    return "msr3d_bf16_skinny_lowrank" if M <= 32 else "msr3d_bf16_skinny_lowrank_wide"


def skinny_project(h, mods, swiglu, src):
    """The projections `mods` of the same activations h (M <= 64, K) bf16 contiguous -> list of (M, N) bf16 (one tensor
    with swiglu), one launch per input group, on weight source `src`, which states: `prepare(module)` (or None), what
    comes first; `r_row(h, m0, M, K, dev)` -> (tensors to keep, the entry's activation operands), the group's r-row
    launch; `job(module, K, C)`, a member's job struct (`Job`); `R`; `entry(M)`, the entry's name."""
    M, K = h.shape
    dev = h.device
    outs, calls, prepare = [None] * len(mods), {}, src.prepare
    for j, m in enumerate(mods):
        if prepare is not None:
            prepare(m)
        calls.setdefault(id(m._group) if m._group is not None else id(m), []).append(j)
    if swiglu and len(calls) != 1:
        # gate and up without a shared low-rank activation (modules moved to the device after construction leave
        # their input group): two products and the stand-alone SwiGLU launch
        gate, up = skinny_project(h, mods, False, src)
        act = torch.empty_like(gate)
        with torch.cuda.device(dev):
            call("msr3d_swiglu_fwd", gate.numel(), ptr(gate), ptr(up), ptr(act), current_stream_ptr(dev))
        return [act]
    R, entry, job = src.R, src.entry(M), src.job
    for js in calls.values():
        held = None                                         # (the last group's activations go before this one's come)
        held, operands = src.r_row(h, mods[js[0]], M, K, dev)
        jobs = (src.Job * len(js))()
        for n, j in enumerate(js):
            m = mods[j]
            if not (swiglu and n == 1):
                outs[j] = torch.empty((M, m.out_features), dtype=torch.bfloat16, device=dev)
            jobs[n] = job(m, K, outs[j].data_ptr() if outs[j] is not None else 0)
        with torch.cuda.device(dev):
            call(entry, M, K, R, *operands, len(js), jobs, int(swiglu), current_stream_ptr(dev))
    return outs


class SkinnyProducts:
    """The products of one decode step on weight source `src`."""

    def __init__(self, src):
        self.src = src

    def project(self, h, mods):
        return skinny_project(h, mods, False, self.src)

    def gated(self, h, gate, up):
        return skinny_project(h, (gate, up), True, self.src)[0]

    @staticmethod
    def head(h, lm_head):
        """The head is a FrozenLinear (bf16, no pair, no e4m3 image): the R = 0 form of the bf16 entry for every source."""
        lm_head._sync()
        M, K, V = h.shape[0], lm_head.in_features, lm_head.out_features
        logits = torch.empty((M, V), dtype=torch.bfloat16, device=h.device)
        job = (_lib.SkinnyJob * 1)(_lib.SkinnyJob(lm_head.weight.data_ptr(), K, 0, 0, logits.data_ptr(), V, V))
        with torch.cuda.device(h.device):
            call(skinny_entry(M), M, K, 0, ptr(h), K, ptr(None), 0, 1, job, 0, current_stream_ptr(h.device))
        return logits


def _a_operand(m0):
    """The A rows of a group's r-row product: the members' stacked images, or the module's own."""
    return m0._group["a_cat"] if m0._group is not None else m0._shadows(forward=True)[0]


def _eval_rows(h, refusal):
    """The guard of the wide forms that build no autograd graph -> h as (rows, K) bf16 contiguous."""
    if torch.is_grad_enabled() and h.requires_grad:
        raise RuntimeError(refusal)
    if not h.is_cuda:
        raise RuntimeError("LoRALinear runs on the GPU only (no CPU fallback)")
    x2 = h.to(torch.bfloat16).reshape(-1, h.shape[-1])
    return x2 if x2.is_contiguous() else x2.contiguous()


class SeparateProducts(ModuleProducts):
    """lora="separate": W and the low-rank pair side by side, the training graph's arithmetic.  Wide: ModuleProducts as
    it stands.  Skinny: the r-row product s h A^T first, then W | B2 of every member with R = 64."""
    R, Job, entry, prepare = PAD_R, _lib.SkinnyJob, staticmethod(skinny_entry), staticmethod(LoRALinear._sync_weight_t)

    def __init__(self):
        self.skinny = SkinnyProducts(self)

    @staticmethod
    def r_row(h, m0, M, K, dev):
        a_op = _a_operand(m0)
        u = torch.empty((M, PAD_R), dtype=torch.bfloat16, device=dev)
        _skinny(M, a_op.shape[0], K, h, a_op, u, PAD_R, m0.scaling, dev)
        return u, (ptr(h), K, ptr(u), PAD_R)

    @staticmethod
    def job(m, K, C):
        return _lib.SkinnyJob(m.weight.data_ptr(), K, m._shadows(forward=True)[1].data_ptr(), PAD_R, C, m.out_features,
                              m.out_features)


class MergedModuleProducts(ModuleProducts):
    """lora="merged": every product on its plane bf16(W + s B A) alone (planes: LoRALlamaStack.merged_weights(), which
    states cost and staleness) -- the same launches with R = 0, no r-row product and no low-rank activation.  Wide: ONE
    tiled product per projection, msr3d_bf16_gemm_lowrank with R = 0.  Evaluation only: no autograd graph is built, and
    a call that would need one (gradients enabled on activations that require grad) raises."""
    R, Job, entry, prepare = 0, _lib.SkinnyJob, staticmethod(skinny_entry), None
    r_row = staticmethod(lambda h, m0, M, K, dev: (None, (ptr(h), K, ptr(None), 0)))       # (no r-row launch: P2 NULL)

    def __init__(self, planes):
        self.planes = planes
        self.skinny = SkinnyProducts(self)
        self.fused = FusedSkinnyProducts(self)              # (step="fused": the same planes, fewer launches)

    def project(self, h, mods):
        x2 = _eval_rows(h, "MergedModuleProducts: merged weights are for evaluation (no backward); call under "
                           "torch.no_grad() or use lora='separate'")
        outs = []
        for m in mods:
            y = torch.empty((x2.shape[0], m.out_features), dtype=torch.bfloat16, device=h.device)
            _gemm(x2.shape[0], m.out_features, m.in_features, 0, x2, m.in_features, self.planes[m], m.in_features, None, 0,
                  None, 0, y, m.out_features, False, 1.0, h.device)
            outs.append(y)
        return outs

    def gated(self, h, gate, up):
        g, u = self.project(h, (gate, up))
        return _SwiGLUFn.apply(g, u)

    def job(self, m, K, C):
        return _lib.SkinnyJob(self.planes[m].data_ptr(), K, 0, 0, C, m.out_features, m.out_features)


# step="fused" runs its fused launches up to this many live rows; above, the step is the split sequence (the same bits).
# A prologue launch normalises its activations again in every workgroup (and walks all M rows for their rstd first), which
# grows with M while the launches it saves do not: measured (profiles/generate_fused.txt) faster than split up to 10 rows,
# level with it at 15 and 8-12 % slower at 20, where the product takes its second activation tile.
FUSED_MAX_ROWS = 15


class FusedSkinnyProducts:
    """step="fused": MergedModuleProducts.skinny with the launches around each product folded into it -- ONE call of
    msr3d_bf16_skinny_fused per product, R = 0 (include/msr3d_hip.h states the three pieces and why each gives the bits of
    the launch it replaces).  `norm` = (weight, eps): the product reads RMSNorm(h) weight; `residual`: the output is
    bf16(residual + product), a fresh tensor; `rope` (q | k | v on a bf16 cache) = (H, D, pos, len, cos, sin, table_rows,
    k_plane, v_plane, Tmax): q comes back rotated, k and v go into the planes alone."""

    def __init__(self, src):
        self.src = src

    def _call(self, h, jobs, swiglu, norm=None, residual=None, rope=None):
        M, K = h.shape
        nw, eps = norm if norm is not None else (None, 0.0)
        tail = (rope[0], rope[1], *(ptr(t) for t in rope[2:6]), rope[6], ptr(rope[7]), ptr(rope[8]), rope[9]) \
            if rope is not None else (0, 0, ptr(None), ptr(None), ptr(None), ptr(None), 0, ptr(None), ptr(None), 0)
        with torch.cuda.device(h.device):
            call("msr3d_bf16_skinny_fused", M, K, 0, ptr(h), K, ptr(None), 0, len(jobs), jobs, int(swiglu), ptr(nw),
                 ctypes.c_float(eps), ptr(residual), residual.shape[1] if residual is not None else 0, *tail,
                 current_stream_ptr(h.device))

    def project(self, h, mods, norm=None, residual=None, rope=None):
        """-> one (M, N) tensor per module; under `rope` q alone."""
        M, K = h.shape
        outs = [torch.empty((M, m.out_features), dtype=torch.bfloat16, device=h.device)
                for m in (mods[:1] if rope is not None else mods)]
        jobs = (_lib.SkinnyJob * len(mods))()
        for n, m in enumerate(mods):
            jobs[n] = self.src.job(m, K, outs[n].data_ptr() if n < len(outs) else 0)
        self._call(h, jobs, False, norm, residual, rope)
        return outs

    def gated(self, h, gate, up, norm):
        M, K = h.shape
        act = torch.empty((M, gate.out_features), dtype=torch.bfloat16, device=h.device)
        jobs = (_lib.SkinnyJob * 2)(self.src.job(gate, K, act.data_ptr()), self.src.job(up, K, 0))
        self._call(h, jobs, True, norm)
        return act

    def head(self, h, lm_head, norm):
        lm_head._sync()
        M, K, V = h.shape[0], lm_head.in_features, lm_head.out_features
        logits = torch.empty((M, V), dtype=torch.bfloat16, device=h.device)
        self._call(h, (_lib.SkinnyJob * 1)(_lib.SkinnyJob(lm_head.weight.data_ptr(), K, 0, 0, logits.data_ptr(), V, V)),
                   False, norm)
        return logits


class E4m3Products(ModuleProducts):
    """weights="e4m3": a base="fp8" stack on its own e4m3 images (csrc/llm_decode_fp8.hip).  Skinny: the bf16 step's input
    groups and launch count at half the weight bytes -- the r-row launch also writes the e4m3 codes of h and their row
    scales, the product streams weight_q / weight_scale of every member.  Wide: every LoRA projection multiplies on
    e4m3, whatever the number of token rows: from 128 up the modules' own forward (msr3d_fp8_gemm_lowrank) -- the stack's
    full forward bit for bit; below, where LoRALinear falls back to its bf16 plane, slabs of at most 64 rows on the skinny
    form.  The two kernels add the same exact e4m3 products in different orders: a walk of fewer than 128 rows may
    differ from a larger one in last bits.
    scratch: a dict that keeps (u, codes, scales) per (M, K, device) between launches, or None for fresh tensors (the
    slab walk).  Nothing reads them after the group's second launch, and an engine's launches are ordered on one
    stream, so a step allocates its outputs alone (at a few rows a step is bounded by its host time)."""
    R, Job, entry = PAD_R, _lib.Fp8SkinnyJob, staticmethod(lambda M: "msr3d_fp8_skinny_lowrank")

    def __init__(self, scratch=None):
        self.scratch = scratch                              # (None: an engine's source -- its step's side keeps one)
        self.skinny = SkinnyProducts(self if scratch is not None else E4m3Products({}))

    @staticmethod
    def prepare(m):
        m._sync_weight_t()                                  # (requantises weight_q when the bf16 weight was written)
        if m.base != "fp8" or m.weight_q is None:
            raise RuntimeError("weights='e4m3': a projection without an e4m3 image (base='fp8' modules on the GPU only)")

    def r_row(self, h, m0, M, K, dev):
        a_op, scratch = _a_operand(m0), self.scratch
        buf = scratch.get((M, K, dev)) if scratch is not None else None
        if buf is None:
            buf = (torch.empty((M, PAD_R), dtype=torch.bfloat16, device=dev),
                   torch.empty((M, K), dtype=torch.uint8, device=dev), torch.empty((M,), dtype=torch.float32, device=dev))
            if scratch is not None:
                scratch[(M, K, dev)] = buf
        u, hq, sh = buf
        with torch.cuda.device(dev):
            call("msr3d_bf16_gemm_skinny_quant", M, a_op.shape[0], K, ptr(h), K, ptr(a_op), K, ptr(u), PAD_R, PAD_R,
                 ctypes.c_float(m0.scaling), ptr(hq), K, ptr(sh), current_stream_ptr(dev))
        return buf, (ptr(hq), K, ptr(sh), ptr(u), PAD_R)

    @staticmethod
    def job(m, K, C):
        return _lib.Fp8SkinnyJob(m.weight_q.data_ptr(), K, m.weight_scale.data_ptr(), m._shadows(forward=True)[1].data_ptr(),
                                 PAD_R, C, m.out_features, m.out_features)

    def _slabs(self, h, mods, swiglu):
        x2 = _eval_rows(h, "E4m3ModuleProducts: evaluation only (no backward); call under torch.no_grad()")
        cols = None                                         # per output, its slabs in row order
        for s in range(0, x2.shape[0], E4M3_SLAB):
            part = [o for o in skinny_project(x2[s:s + E4M3_SLAB], mods, swiglu, self) if o is not None]
            cols = [[o] for o in part] if cols is None else [c + [o] for c, o in zip(cols, part)]
        return [c[0] if len(c) == 1 else torch.cat(c, 0) for c in cols]

    def project(self, h, mods):
        wide = h.numel() // h.shape[-1] >= E4M3_WIDE_MIN
        return ModuleProducts.project(h, mods) if wide else self._slabs(h, mods, False)

    def gated(self, h, gate, up):
        wide = h.numel() // h.shape[-1] >= E4M3_WIDE_MIN
        return ModuleProducts.gated(h, gate, up) if wide else self._slabs(h, (gate, up), True)[0]
