"""CPU: msr3d_fp8_skinny_lowrank is declared in include/msr3d_hip.h, exported by the library and bound in _lib with the
header's argument list; its job struct has the header's layout; its argument checks answer without a device; and the
`weights` keyword is on every door that leads to the engine."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_exported_and_bound():
    from msr3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "msr3d_hip.h")).read()
    m = re.search(r"\bint msr3d_fp8_skinny_lowrank\(([^;]*)\);", header)
    assert m, "not declared"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == len(_lib._SIGNATURES["msr3d_fp8_skinny_lowrank"]) == 12
    assert "msr3d_fp8_skinny_lowrank" in _lib.exported_symbols()
    assert hasattr(_lib.load(), "msr3d_fp8_skinny_lowrank")
    # the struct: Wq, ldw, sw, B2, ldb2, C, ldc, N with C's natural padding
    fields = re.search(r"typedef struct \{([^}]*)\} msr3d_fp8_skinny_job_t;", header).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields))
    assert names == [f[0] for f in _lib.Fp8SkinnyJob._fields_] == ["Wq", "ldw", "sw", "B2", "ldb2", "C", "ldc", "N"]
    assert ctypes.sizeof(_lib.Fp8SkinnyJob) == 56 and _lib.Fp8SkinnyJob.sw.offset == 16 and _lib.Fp8SkinnyJob.C.offset == 40


def test_argument_checks_answer_without_a_device():
    from msr3d_amd import _lib
    h, null = _lib.load(), ctypes.c_void_p(0)
    job = (_lib.Fp8SkinnyJob * 1)()
    assert h.msr3d_fp8_skinny_lowrank(1, 128, 0, null, 128, null, null, 0, 1, job, 0, null) == -22     # null operands
    assert h.msr3d_fp8_skinny_lowrank(65, 128, 0, null, 128, null, null, 0, 1, job, 0, null) == -22    # M > 64
    assert h.msr3d_fp8_skinny_lowrank(1, 64, 0, null, 128, null, null, 0, 1, job, 0, null) == -22      # K % 128
    assert h.msr3d_fp8_skinny_lowrank(1, 128, 0, null, 128, null, null, 0, 4, job, 0, null) == -22     # njobs > 3
    assert h.msr3d_fp8_skinny_lowrank(1, 128, 0, null, 128, null, null, 0, 0, None, 0, null) == 0      # no job: nothing to do


def test_the_weights_keyword_is_on_every_door():
    from msr3d_amd.llm import LoRALlamaStack
    from msr3d_amd.llm import generate as G
    from msr3d_amd.model.msr3d_full import MSR3DFullStep
    for fn in (G.CachedDecoder.__init__, G.generate, G.predict_answers, LoRALlamaStack.generate, LoRALlamaStack.predict_answers,
               MSR3DFullStep.generate, MSR3DFullStep.predict_answers):
        p = inspect.signature(fn).parameters
        assert "weights" in p and p["weights"].default == "bf16", fn
