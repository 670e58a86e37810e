"""CPU: the C-ABI library loads and exports every symbol include/msr3d_hip.h declares;
argument validation works without a device (no compute calls)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_exported():
    from msr3d_amd import _lib
    h = _lib.load()
    header = open(os.path.join(ROOT, "include", "msr3d_hip.h")).read()
    declared = set(re.findall(r"\b(msr3d_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    for sym in declared:
        assert hasattr(h, sym), f"{sym} declared in the header but not exported"
    assert declared == set(_lib.exported_symbols())
    assert h.msr3d_abi_version() == int(re.search(r"#define MSR3D_ABI_VERSION (\d+)", header).group(1)) >= 2


def test_invalid_arguments_are_rejected_without_a_device():
    from msr3d_amd import _lib
    h = _lib.load()
    null = ctypes.c_void_p(0)
    # n <= 0 / null pointers -> MSR3D_EINVAL, never a crash or an exit()
    assert h.msr3d_furthest_point_sampling(1, 0, 4, null, null, null, null) == -22
    assert h.msr3d_furthest_point_sampling(1, 8, 4, null, null, null, null) == -22
    assert h.msr3d_furthest_point_sampling(0, 8, 4, null, null, null, null) == 0      # empty batch
    assert h.msr3d_ball_query(-1, 8, 4, ctypes.c_float(0.2), 4, null, null, null, null) == -22
    assert h.msr3d_group_points(1, 1, 8, 2, 2, null, null, null, null) == -22
    assert h.msr3d_status_string(-22) == b"invalid argument"
    assert h.msr3d_status_string(0) == b"ok"
    # empty problems are a successful no-op
    assert h.msr3d_gather_points(0, 3, 8, 4, null, null, null, null) == 0


def test_struct_launcher_fills_fields_and_names_them_in_a_failure():
    """_lib.fill / _lib.launch, the one door of every struct-taking entry: a tensor gives its data pointer, a c_void_p its
    value, None is NULL, numbers pass; a non-zero status raises with the entry's name and the struct's non-zero fields."""
    import pytest
    import torch
    from msr3d_amd import _lib
    t = torch.zeros(8)
    s = _lib.fill(_lib.StripGemm(), dict(M=12, a0=t, a1=ctypes.c_void_p(4096), a2=None, eps1=0.5, salt1=7))
    assert (s.M, s.a0, s.a1, s.a2, s.eps1, s.salt1) == (12, t.data_ptr(), 4096, None, 0.5, 7)
    assert s.N == 0 and s.W is None                       # untouched fields stay zero
    arr = _lib.fill((_lib.GemmProblem * 2)(), [dict(M=3, A=t, bias=None, beta=1.0), dict(M=5, B=ctypes.c_void_p(64), beta=0.25)])
    assert (arr[0].M, arr[0].A, arr[0].bias, arr[0].beta) == (3, t.data_ptr(), None, 1.0)
    assert (arr[1].M, arr[1].A, arr[1].B, arr[1].beta) == (5, None, 64, 0.25)

    class Stub:
        calls = []

        def msr3d_strip_gemm_f32(self, ref, stream):
            self.calls.append((ref._obj.M, stream))
            return 0

        def msr3d_gemm_multi_f32(self, n, probs, stream):
            self.calls.append((n, probs[1].M, stream))
            return -22
    _lib.launch("msr3d_strip_gemm_f32", s, 99, lib=Stub())          # a struct goes by reference; status 0: no error
    with pytest.raises(RuntimeError) as e:
        _lib.launch("msr3d_gemm_multi_f32", arr, 99, lib=Stub())    # an array goes as (count, array)
    assert Stub.calls == [(12, 99), (2, 5, 99)]
    msg = str(e.value)
    assert "msr3d_gemm_multi_f32(" in msg and "invalid argument" in msg
    assert f"M=3, A={t.data_ptr()}, beta=1.0; M=5, B=64, beta=0.25" in msg
    with pytest.raises(RuntimeError, match=r"msr3d_x failed: invalid argument \(status -22\)"):
        _lib.call("msr3d_x", 1, lib=type("L", (), {"msr3d_x": staticmethod(lambda n: -22)})())


def test_no_oracle_import_in_product():
    """The product package must never import, link or call the oracle."""
    pkg = os.path.join(ROOT, "msr3d_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(d, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f
                assert "libpn2_oracle" not in src and "pn2o_" not in src, f
