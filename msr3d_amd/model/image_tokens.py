"""The 2D image branch of `MSR3D.build_embeds` (the reference's model/msr3d/msr3d.py:98-100 `llm_proj_img`,
:233-252): every image of a sample stands for ONE placeholder token of the prompt, whose embedding is replaced by
`llm_proj_img(pooled image feature)` before the scene tokens go in.

The frozen ConvNeXt backbone stays outside, as the tokenizer does: it runs under no_grad and its pooled output is
cacheable, so the branch starts there -- `img_fts (B, N, C)` fp32, one `(out_channels,)` vector per image slot
(modules/vision/timm.py:72-77,112-116 with `pooling: avg`; 1024 for convnext_base), and `img_masks (B, N)` bool.

Two modes:
  "interleaved"  the 'msr3d_imgs' branch (msr3d.py:234-245): the real images are the slots whose mask is set, in
                 row-major order (`pixel_values[img_mask.bool()]`); the k-th real image's token replaces the embedding of
                 the k-th position where input_ids == img_sp_token, row-major over (B, T).  attention_mask is not touched.
  "single"       the `img_tokens` branch (msr3d.py:247-252,261-266): N = 1, every slot is a source, masked or not; the
                 k-th placeholder takes the k-th slot's token and attention_mask there becomes img_masks of the slot.
                 The reference's masking of the situation text in this branch (`find_subsequence`, msr3d.py:254-267) is
                 token-level prompt assembly and stays with the caller's attention_mask.
A batch whose placeholder count differs from its source count gets the first min(placeholders, sources) pairs; surplus
placeholders keep their embedding-table rows, nothing is read or written out of bounds, and the counts stay on the device.

The reference's torch.where and boolean-mask compaction are a host sync each; csrc/image_tokens.hip builds both maps on
the device and projects, casts and scatters in one launch (f32-input MFMA: the reference runs this Linear in fp32 outside
autocast and only then casts)."""
import ctypes

import torch

from .scene_embeds import _DTYPE_CODE

IMG_SP_TOKEN = 30861     # vicuna id of the image placeholder (msr3d.py:213)
MODES = {"interleaved": 0, "single": 1}


def scatter_image_tokens(inputs_embeds, attention_mask, input_ids, img_tokens, img_masks, img_sp_token=IMG_SP_TOKEN,
                         mode="interleaved"):
    """The torch mirror of the index work (runs anywhere, no host sync; the documentation of the kernels and the CPU
    fallback): img_tokens (B, N, E) are the ALREADY projected tokens of every slot (`llm_proj_img(img_fts)`), cast here to
    inputs_embeds' dtype.  cumsum ranks the placeholders, a stable sort of the slot mask compacts the sources, and the
    first min(placeholders, sources) pairs are written.  Returns (inputs_embeds, attention_mask) as new tensors;
    attention_mask comes back unchanged in "interleaved" mode."""
    if mode not in MODES:
        raise ValueError(f"image_mode must be one of {sorted(MODES)}")
    B, T = input_ids.shape
    cap = img_tokens.shape[0] * img_tokens.shape[1]
    if cap == 0:
        return inputs_embeds.clone(), attention_mask.clone() if attention_mask is not None else None
    hit = input_ids == img_sp_token                                     # (B, T)
    rank = torch.cumsum(hit.reshape(-1).to(torch.int64), 0) - 1        # k-th placeholder -> k
    slot_mask = img_masks.reshape(-1).bool()
    if mode == "interleaved":
        order = torch.argsort((~slot_mask).to(torch.int8), stable=True)     # the set slots first, in slot order
        n_src = slot_mask.sum()
    else:
        order = torch.arange(cap, device=input_ids.device)
        n_src = torch.full((), cap, dtype=torch.int64, device=input_ids.device)
    live = (hit.reshape(-1) & (rank < n_src)).reshape(B, T)            # surplus placeholders stay as they are
    slot = order.index_select(0, rank.clamp(min=0, max=cap - 1))        # (B*T,) source slot of every position
    rows = img_tokens.reshape(cap, -1).to(inputs_embeds.dtype).index_select(0, slot).reshape(B, T, -1)
    out_embeds = torch.where(live.unsqueeze(-1), rows, inputs_embeds)
    out_mask = attention_mask
    if attention_mask is not None:
        out_mask = attention_mask.clone()
        if mode == "single":
            m = slot_mask.index_select(0, slot).reshape(B, T).to(attention_mask.dtype)
            out_mask = torch.where(live, m, attention_mask)
    return out_embeds, out_mask


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _launch(inputs_embeds, attention_mask, input_ids, img_fts, img_masks, weight, bias, img_sp_token, mode):
    """map + forward (msr3d_image_project_scatter) -> (dest, src, counts, the fp32 features it read)."""
    from .. import _lib
    if mode not in MODES:
        raise ValueError(f"image_mode must be one of {sorted(MODES)}")
    B, T = input_ids.shape
    if img_fts.dim() != 3 or img_fts.shape[0] != B or tuple(img_masks.shape) != tuple(img_fts.shape[:2]):
        raise RuntimeError("img_fts (B, N, C) and img_masks (B, N) expected")
    N, C = img_fts.shape[1], img_fts.shape[2]
    E = inputs_embeds.shape[-1]
    if mode == "single" and N != 1:
        raise RuntimeError('image_mode "single" takes one image slot per sequence (N = 1)')
    if not (inputs_embeds.is_cuda and inputs_embeds.is_contiguous() and input_ids.dtype == torch.int64):
        raise RuntimeError("project_scatter_images_: contiguous GPU tensors and int64 ids expected")
    if inputs_embeds.dtype not in _DTYPE_CODE:
        raise RuntimeError("inputs_embeds must be fp32, fp16 or bf16")
    if attention_mask is not None and (attention_mask.dtype != torch.int64 or not attention_mask.is_contiguous()):
        raise RuntimeError("attention_mask must be contiguous int64")
    if tuple(weight.shape) != (E, C):
        raise RuntimeError(f"llm_proj_img weight {tuple(weight.shape)} does not map {C} features to {E}")
    dev = input_ids.device
    fts = img_fts.detach().reshape(B * N, C).float().contiguous()
    msk = img_masks.reshape(B * N).to(torch.bool).contiguous().view(torch.uint8)
    w = weight.detach()
    w = w if w.is_contiguous() else w.contiguous()
    b = bias.detach().contiguous() if bias is not None else None
    dest = torch.empty(max(B * N, 1), dtype=torch.int32, device=dev)
    src = torch.empty(max(B * N, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = lib.msr3d_image_project_scatter(B, T, N, C, E, MODES[mode], _p(input_ids.contiguous()), int(img_sp_token),
                                             _p(fts), _p(msk), _p(w), 0 if w.dtype == torch.float32 else 1, _p(b),
                                             _DTYPE_CODE[inputs_embeds.dtype], _p(inputs_embeds), _p(attention_mask),
                                             _p(dest), _p(src), _p(cnt), _lib.current_stream_ptr(dev))
    _lib.check(rc, "msr3d_image_project_scatter")
    return dest, src, cnt, fts


def image_project_grad(d_inputs_embeds, dest, src, counts, img_fts, d_weight, d_bias, accumulate=False, clear_rows=True):
    """msr3d_image_project_grad through the map a forward call left: d_weight (E, C) / d_bias (E) fp32 (+)= the weight /
    bias gradient of the placeholder rows of d_inputs_embeds (B, T, E; read in its dtype), k ascending; clear_rows then
    zeroes those rows IN PLACE.  img_fts: the (B*N, C) fp32 features of the forward call."""
    from .. import _lib
    g = d_inputs_embeds
    if not (g.is_cuda and g.is_contiguous() and g.dtype in _DTYPE_CODE):
        raise RuntimeError("d_inputs_embeds must be a contiguous fp32 / fp16 / bf16 GPU tensor")
    E = g.shape[-1]
    C = img_fts.shape[-1]
    if tuple(d_weight.shape) != (E, C) or d_weight.dtype != torch.float32 or not d_weight.is_contiguous():
        raise RuntimeError("d_weight must be a contiguous fp32 (E, C) tensor")
    cap = img_fts.numel() // C
    with torch.cuda.device(g.device):
        rc = _lib.load().msr3d_image_project_grad(cap, C, E, g.numel() // E, _p(dest), _p(src), _p(counts), _p(img_fts),
                                                  _DTYPE_CODE[g.dtype], _p(g), _p(d_weight), _p(d_bias),
                                                  1 if accumulate else 0, 1 if clear_rows else 0,
                                                  _lib.current_stream_ptr(g.device))
    _lib.check(rc, "msr3d_image_project_grad")


def project_scatter_images_(inputs_embeds, attention_mask, input_ids, img_fts, img_masks, llm_proj_img,
                            img_sp_token=IMG_SP_TOKEN, mode="interleaved", validate=False):
    """In-place HIP form (msr3d_image_project_scatter): two launches, no host sync.  inputs_embeds (B, T, E) f32 / f16 /
    bf16 contiguous, attention_mask (B, T) int64 or None (written in "single" mode only), input_ids (B, T) int64,
    img_fts (B, N, C) f32, img_masks (B, N) bool, llm_proj_img an fp32 nn.Linear(C, E) with C % 32 == 0, E % 128 == 0.
    Returns the device int32 pair (placeholders found, sources).

    INFERENCE / no-grad only: the kernel writes through raw pointers, autograd does not see it.  Called with gradients
    enabled on a projection that requires grad it raises -- training uses project_scatter_images_train_.
    validate=True syncs and raises if the two counts differ, as the reference's indexed assignment does."""
    w, b = llm_proj_img.weight, llm_proj_img.bias
    if torch.is_grad_enabled() and (w.requires_grad or (b is not None and b.requires_grad) or inputs_embeds.requires_grad):
        raise RuntimeError("project_scatter_images_ has no autograd: use project_scatter_images_train_ "
                           "(or run under torch.no_grad() for inference)")
    _, _, cnt, _ = _launch(inputs_embeds, attention_mask, input_ids, img_fts, img_masks, w, b, img_sp_token, mode)
    if validate:
        found, sources = (int(v) for v in cnt.tolist())
        if found != sources:
            raise RuntimeError(f"{found} image placeholders in input_ids but {sources} images")
    return cnt


class _ProjectScatterImages(torch.autograd.Function):
    """The training-time form: in place like msr3d.py:243-245, with the gradient the reference's Linear + indexed
    assignment have -- d llm_proj_img from the placeholder rows of d inputs_embeds, none for the overwritten embeddings,
    none for img_fts (the encoder is frozen).  The node ALWAYS delivers a gradient for llm_proj_img, zeros when the batch
    has no image: a probe on an image-free batch must not file the parameter as unused."""

    @staticmethod
    def forward(ctx, inputs_embeds, weight, bias, attention_mask, input_ids, img_fts, img_masks, token, mode):
        dest, src, cnt, fts = _launch(inputs_embeds, attention_mask, input_ids, img_fts, img_masks, weight, bias, token, mode)
        ctx.mark_dirty(inputs_embeds)
        ctx.save_for_backward(dest, src, cnt, fts)
        ctx.weight, ctx.bias = weight, bias                # (the Parameter objects themselves: they carry the engine)
        return inputs_embeds

    @staticmethod
    def backward(ctx, g):
        from .. import hipops
        dest, src, cnt, fts = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        if ctx.needs_input_grad[0]:
            g = g.clone(memory_format=torch.contiguous_format)          # its placeholder rows are cleared below
        elif not g.is_contiguous():
            g = g.contiguous()
        want_w = ctx.needs_input_grad[1]
        want_b = bias is not None and ctx.needs_input_grad[2]
        direct = None
        if want_w and (want_b or bias is None):
            direct = hipops._direct_targets(*((weight, bias) if bias is not None else (weight,)))
        if direct is not None:
            # on the flat-gradient engine the .grad are views of the flat buffer: the kernel ADDS into them
            dW, db, acc = weight.grad, (bias.grad if bias is not None else None), True
        else:
            dW = torch.empty_like(weight, memory_format=torch.contiguous_format)
            db = torch.empty_like(bias) if bias is not None else None
            acc = False
        image_project_grad(g, dest, src, cnt, fts, dW, db, accumulate=acc, clear_rows=ctx.needs_input_grad[0])
        d_in = g if ctx.needs_input_grad[0] else None
        if direct is not None:
            hipops._direct_done(direct)
            return (d_in,) + (None,) * 8
        return d_in, (dW if want_w else None), (db if want_b else None), None, None, None, None, None, None


def project_scatter_images_train_(inputs_embeds, attention_mask, input_ids, img_fts, img_masks, llm_proj_img,
                                  img_sp_token=IMG_SP_TOKEN, mode="interleaved"):
    """In-place HIP form WITH autograd (where msr3d.py:233-252 sits in the training forward): returns inputs_embeds;
    gradients reach llm_proj_img -- straight into the flat-buffer views when the flat-gradient engine owns them."""
    return _ProjectScatterImages.apply(inputs_embeds, llm_proj_img.weight, llm_proj_img.bias, attention_mask, input_ids,
                                       img_fts, img_masks, int(img_sp_token), mode)
