"""What of prompt_cache="shared" can be checked without a GPU: the loaded library exports msr3d_attn_decode_shared under
the header's ABI version, the binding declares it with the header's argument list, and the engine's argument check
knows the option."""
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msr3d_hip.h")


def test_the_library_exports_the_entry_under_abi_39():
    from msr3d_amd import _lib
    h = _lib.load()
    assert hasattr(h, "msr3d_attn_decode_shared")
    header = open(HEADER).read()
    assert int(re.search(r"#define MSR3D_ABI_VERSION (\d+)", header).group(1)) == 39
    assert _lib.ABI_VERSION == h.msr3d_abi_version() == 39


def test_the_binding_has_one_argument_type_per_header_argument():
    from msr3d_amd import _lib
    header = open(HEADER).read()
    decl = re.search(r"int msr3d_attn_decode_shared\(([^;]*)\);", header).group(1)
    assert len(_lib._SIGNATURES["msr3d_attn_decode_shared"]) == len(decl.split(",")) == 22


def test_the_engine_refuses_an_unknown_prompt_cache():
    from msr3d_amd.llm.generate import CachedDecoder, KVCache
    with pytest.raises(ValueError, match="prompt_cache is 'rows' or 'shared'"):
        CachedDecoder(object(), prompt_cache="x")                   # (checked before the stack is looked at)
    with pytest.raises(ValueError, match="layout"):
        KVCache(1, 5, 8, 2, 64, "cpu", layout="x")
