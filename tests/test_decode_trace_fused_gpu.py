"""The launch sequence of a step="fused" decode step, recorded at the library's door with tests/test_decode_trace_gpu.py's
`record`: five entry calls a layer and one for the head, no norm and no append launch; six a layer on an e4m3 cache, which
keeps its append; above products.FUSED_MAX_ROWS live rows the split sequence; and step="split" records what it always did."""
import pytest
import torch

from tests.generate_helpers import prompt
from tests.test_decode_trace_gpu import (BEAMS, D, H, HID, INTER, NEW, NL, RMS, SKINNY, T, _coarse, _grouped, _step,
                                         record)

pytestmark = pytest.mark.gpu

FUSED = "msr3d_bf16_skinny_fused"
APPEND, APPEND_E4M3 = "msr3d_rope_kv_append", "msr3d_rope_kv_append_e4m3"


def _coarse_fused(name, args):
    """_coarse, with (njobs, swiglu) of the fused entry where the plain entries have them."""
    return (*_coarse(name, args), args[7], args[9]) if name == FUSED else _coarse(name, args)


def _one_step(B, layout="rows", **engine_kw):
    """reserve, prefill, expand outside the recording; one step of B x 5 rows inside it."""
    from msr3d_amd.llm.generate import CachedDecoder
    net, emb = _grouped("bf16")
    eng = CachedDecoder(net, lora="merged", prompt_cache=layout, **engine_kw)
    x, keep = prompt(0, B=B)
    eng.reserve(BEAMS, NEW)
    eng.prefill(x.cuda(), keep.cuda())
    eng.expand(BEAMS)
    tok = emb[torch.arange(B * BEAMS).cuda() + 3].contiguous()
    trace = record(lambda: eng.step(tok))
    return [_coarse_fused(n, a) for n, a in trace]


def _fused_step(N, attend):
    layer = ([(FUSED, N, HID, 0, 3, 0)] + attend + [(FUSED, N, HID, 0, 1, 0), (FUSED, N, HID, 0, 2, 1), (FUSED, N, INTER, 0, 1, 0)])
    return layer * NL + [(FUSED, N, HID, 0, 1, 0)]


@pytest.mark.parametrize("layout", ["rows", "shared"])
def test_a_fused_step_is_five_calls_a_layer_and_the_head(layout):
    N = 3 * BEAMS                                     # 15 rows
    got = _one_step(3, layout, step="fused")
    attend = [("msr3d_attn_decode_shared", 3, BEAMS, T, NEW, H, D)] if layout == "shared" else \
        [("msr3d_attn_decode", N, T + NEW, H, D)]
    assert got == _fused_step(N, attend), "\n".join(map(str, got))
    names = [r[0] for r in got]
    assert len(got) == 5 * NL + 1 == 11
    assert RMS not in names and APPEND not in names and not set(SKINNY) & set(names)


@pytest.mark.parametrize("kv_kernels", [True, False])
def test_an_e4m3_cache_keeps_its_append_six_calls_a_layer(kv_kernels):
    N = 3 * BEAMS
    got = _one_step(3, "rows", step="fused", kv="e4m3", kv_kernels=kv_kernels)
    if kv_kernels:
        attend = [(APPEND_E4M3, N, H, D, T + NEW), ("msr3d_attn_decode_e4m3", N, T + NEW, H, D)]
    else:
        attend = [(APPEND, N, H, D, T + NEW), ("msr3d_attn_decode", N, T + NEW, H, D)]
    assert got == _fused_step(N, attend), "\n".join(map(str, got))
    assert len(got) == 6 * NL + 1 and RMS not in [r[0] for r in got]


def test_above_the_fallback_row_count_the_step_is_the_split_sequence():
    from msr3d_amd.llm.products import FUSED_MAX_ROWS
    B = FUSED_MAX_ROWS // BEAMS + 1
    if B * BEAMS <= 64:                               # (a constant of 64 would mean: no fallback, nothing to record)
        assert _one_step(B, step="fused") == _step("merged", "rows", B, BEAMS)
    # and the largest row count below it is still fused
    B = FUSED_MAX_ROWS // BEAMS
    assert {r[0] for r in _one_step(B, step="fused")} == {FUSED, "msr3d_attn_decode"}


@pytest.mark.parametrize("layout", ["rows", "shared"])
def test_a_split_step_records_what_it_always_did(layout):
    assert _one_step(3, layout) == _step("merged", layout, 3, BEAMS)
    assert _one_step(3, layout, step="split") == _step("merged", layout, 3, BEAMS)
