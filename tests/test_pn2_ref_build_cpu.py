"""The recipe that compiles the reference's own pointnet2 kernels for cross-checks (oracle/pn2_ref.py): it builds where
the reference is present, exports the nine entry points and records what it compiled; nothing it makes is ever
committed, and its absence is a False, not an exception."""
import os
import subprocess

import pytest

from oracle import pn2_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(
    not pn2_ref.can_build(),
    reason="the reference's pointnet2 device files (%s) or hipcc are not on this machine" % pn2_ref.REFERENCE_ROOT)


@needs_reference
def test_the_recipe_builds_and_records_what_it_built():
    so = pn2_ref.build(force=True)
    assert so == pn2_ref.SO and os.path.exists(so) and pn2_ref.available()
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert len(pn2_ref.SYMBOLS) == 9
    for sym in pn2_ref.SYMBOLS:
        assert sym in names, sym
    info = open(pn2_ref.BUILD_INFO).read()
    for src in ("sampling_gpu.cu", "ball_query_gpu.cu", "group_points_gpu.cu", "interpolate_gpu.cu"):
        line = [ln for ln in info.splitlines() if ln.strip().endswith(src)]
        assert len(line) == 1 and len(line[0].split()[0]) == 64, src          # a sha256 beside each source
    assert "-O3" in info and "gfx950" in info and "-ffp-contract=" not in info and "version" in info.lower()


def test_the_build_passes_no_contraction_flag_and_names_its_limits():
    assert not any("fp-contract" in f or "fast-math" in f or "fmad" in f for f in pn2_ref.FLAGS)
    assert "-O3" in pn2_ref.FLAGS and "-shared" in pn2_ref.FLAGS and "-fPIC" in pn2_ref.FLAGS
    doc = pn2_ref.__doc__
    assert "opt_n_threads(0)" in doc and "check no index" in doc and "exit(-1)" in doc


def test_nothing_under_oracle_ref_is_tracked():
    if not os.path.isdir(os.path.join(ROOT, ".git")):
        pytest.skip("not a git checkout")
    out = subprocess.run(["git", "-C", ROOT, "ls-files", "oracle/_ref"], capture_output=True, text=True, check=True)
    assert out.stdout.strip() == ""
    ignored = subprocess.run(["git", "-C", ROOT, "check-ignore", "-q", "oracle/_ref/libpn2_ref.so"])
    assert ignored.returncode == 0


def test_available_is_false_without_the_library(monkeypatch, tmp_path):
    monkeypatch.setattr(pn2_ref, "SO", str(tmp_path / "_ref" / "libpn2_ref.so"))
    monkeypatch.setattr(pn2_ref, "_lib", None)
    assert pn2_ref.available() is False
    with pytest.raises(RuntimeError, match="is missing"):
        pn2_ref.lib()
