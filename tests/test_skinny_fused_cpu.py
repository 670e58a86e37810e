"""What of step="fused" can be checked without a GPU: the header declares msr3d_bf16_skinny_fused within ABI 39, the binding
carries it with the header's argument list, the library exports it, and the engine checks the keyword's value before it
looks at the stack."""
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msr3d_hip.h")
ENTRY = "msr3d_bf16_skinny_fused"


def _declared(name):
    return re.search(r"int %s\(([^;]*)\);" % name, open(HEADER).read())


def test_the_header_declares_the_entry():
    decl = _declared(ENTRY)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 25
    # skinny_launch's list first, then the prologue, the residual, the rotation block, the stream
    plain = [a.strip() for a in _declared("msr3d_bf16_skinny_lowrank_wide").group(1).split(",")]
    assert args[:len(plain) - 1] == plain[:-1] and args[-1] == plain[-1]
    names = [re.split(r"[ *]", a)[-1] for a in args[len(plain) - 1:-1]]
    assert names == ["norm_w", "eps", "res", "ldres", "H", "D", "pos", "len", "cos_td", "sin_td", "table_rows", "k_plane",
                     "v_plane", "Tmax"]


def test_the_binding_has_one_argument_type_per_header_argument():
    from msr3d_amd import _lib
    assert len(_lib._SIGNATURES[ENTRY]) == len(_declared(ENTRY).group(1).split(",")) == 25
    assert ENTRY in _lib.exported_symbols()


def test_the_abi_version_is_still_39_and_the_library_exports_the_entry():
    from msr3d_amd import _lib
    h = _lib.load()
    assert hasattr(h, ENTRY)
    assert int(re.search(r"#define MSR3D_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 39
    assert _lib.ABI_VERSION == h.msr3d_abi_version() == 39


def test_the_engine_refuses_an_unknown_step_before_it_touches_the_stack():
    from msr3d_amd.llm.generate import CachedDecoder
    for bad in ("x", "both", None, 1):
        with pytest.raises(ValueError, match="step is 'split' or 'fused', not"):
            CachedDecoder(object(), step=bad)
    # (the other keywords' checks still come first, each before the stack is looked at)
    with pytest.raises(ValueError, match="kv is"):
        CachedDecoder(object(), kv="x", step="x")


def test_the_fallback_row_count_is_one_constant_inside_the_entrys_range():
    from msr3d_amd.llm import generate, products
    assert generate.FUSED_MAX_ROWS is products.FUSED_MAX_ROWS
    assert 1 <= products.FUSED_MAX_ROWS <= generate.CachedDecoder.max_rows
