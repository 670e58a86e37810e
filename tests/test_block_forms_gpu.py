"""GPU: the encoder's `fc` on the panel kernel (MSR3D_FC_SPLIT=0, the `f32` mode's form) stays under the same checker as the
default: the encoder against the reference-generated fixture.  The switch is read once per process, so the form runs in a
process of its own."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fc_on_the_panel_kernel_matches_the_fixture():
    env = dict(os.environ, MSR3D_GPU_INPROC="1", MSR3D_FC_SPLIT="0")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_golden_fullsize_gpu.py"), "-q", "-x",
                          "-m", "gpu"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and " passed" in out.stdout, out.stdout[-3000:] + out.stderr[-1000:]
