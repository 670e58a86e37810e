"""The reference's own pointnet2 kernels, compiled for gfx950, as a cross-check of oracle/pn2_oracle.c.

TEST INFRASTRUCTURE ONLY: imported by tests/ and __graft_entry__.build().  Nothing under msr3d_amd/ may import
this, and smoke() / bench.py never do.

`build()` compiles the reference's four device files -- unmodified, read from where the reference lies
(REFERENCE_ROOT) -- with hipcc, against the stand-in headers in oracle/ref_shim/ and the entry points of
oracle/pn2_ref_glue.cpp, into oracle/_ref/libpn2_ref.so, and records what it did in oracle/_ref/BUILD_INFO.txt.
Nothing under oracle/_ref/ is ever committed and nothing of the reference is copied into the tree.  The flags
are the reference's own (-O3, setup.py) and NO -ffp-contract flag: what LLVM does with that source is the thing
being measured.  It is CONTRACT below, read once from `hipcc --cuda-device-only -S` of the same files and flags
and asserted against the running library by tests/test_pn2_reference_gpu.py.

The functions below take and return CUDA torch tensors and do the host-side preparation of the reference's
.cpp files themselves: temp = full(1e10) for FPS (sampling.cpp:66-87), zero-initialised outputs and gradients
everywhere else.

Three properties of the reference's host code limit what may be passed; the wrappers assert the first two
where they can be checked cheaply, the caller owns the rest:
  * opt_n_threads(0) is undefined (log(0) cast to int, then a shift by it; include/cuda_utils.h:15-19), so no
    dimension that sizes a block -- n of FPS, m of ball query, npoints, n of three_nn / three_interpolate, and
    c wherever opt_block_config is used -- may be zero.  No zero-sized dimension is ever passed.
  * the kernels check no index: idx must lie inside the gathered dimension.
  * CUDA_CHECK_ERRORS calls exit(-1) on a failed launch, taking the test process with it: only valid launches
    (b >= 1, sizes that fit a grid) may be issued.
"""
import ctypes
import hashlib
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("MSR3D_REFERENCE_ROOT", "/root/reference")
_EXT_SRC = os.path.join("modules", "third_party", "pointnet2", "_ext_src")
SOURCES = ("sampling_gpu.cu", "ball_query_gpu.cu", "group_points_gpu.cu", "interpolate_gpu.cu")
FLAGS = ("--offload-arch=gfx950", "-x", "hip", "-O3", "-fPIC", "-shared")
REF_DIR = os.path.join(_HERE, "_ref")
SO = os.path.join(REF_DIR, "libpn2_ref.so")
BUILD_INFO = os.path.join(REF_DIR, "BUILD_INFO.txt")
OPS = ("furthest_point_sampling", "gather_points", "gather_points_grad", "ball_query", "group_points",
       "group_points_grad", "three_nn", "three_interpolate", "three_interpolate_grad")
SYMBOLS = tuple("pn2ref_" + o for o in OPS)
# oracle/pn2.py::CONTRACTS key of the contraction this build has (hipcc of ROCm 7.2, -O3, gfx950; see pn2_oracle.c)
CONTRACT = 6

_lib = None


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def source_paths():
    return [os.path.join(REFERENCE_ROOT, _EXT_SRC, "src", s) for s in SOURCES]


def can_build():
    """True where the reference's device files and a hipcc are both present."""
    return _hipcc() is not None and all(os.path.exists(p) for p in source_paths())


def available():
    """True iff the cross-check library has been built (never raises)."""
    return os.path.exists(SO)


def build(force=False):
    """Compile oracle/_ref/libpn2_ref.so and write BUILD_INFO.txt; returns the library's path."""
    if not can_build():
        raise RuntimeError("the reference's pointnet2 device files or hipcc are missing; cannot build " + SO)
    srcs = source_paths()
    glue = os.path.join(_HERE, "pn2_ref_glue.cpp")
    shim = os.path.join(_HERE, "ref_shim")
    deps = srcs + [glue, os.path.abspath(__file__)] + [os.path.join(d, f) for d, _, fs in os.walk(shim) for f in fs]
    if not force and available() and os.path.exists(BUILD_INFO) and \
            os.path.getmtime(SO) >= max(os.path.getmtime(d) for d in deps):
        return SO
    os.makedirs(REF_DIR, exist_ok=True)
    hipcc = _hipcc()
    cmd = [hipcc, *FLAGS, "-I" + shim, "-I" + os.path.join(REFERENCE_ROOT, _EXT_SRC, "include"), *srcs, glue,
           "-o", SO + ".tmp"]
    subprocess.check_call(cmd)
    os.replace(SO + ".tmp", SO)
    ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.strip()
    with open(BUILD_INFO, "w") as f:
        f.write("libpn2_ref.so: the reference's pointnet2 device files compiled for cross-checks; never committed\n")
        f.write("compiler:\n" + "".join("  " + ln + "\n" for ln in ver.splitlines()))
        f.write("flags: " + " ".join(FLAGS) + "  (no -ffp-contract flag: the compiler's default contraction)\n")
        f.write("contraction recorded in oracle/pn2_ref.py: contract %d\n" % CONTRACT)
        f.write("sources (sha256):\n")
        for name, p in zip(SOURCES, srcs):
            with open(p, "rb") as g:
                f.write("  %s  %s\n" % (hashlib.sha256(g.read()).hexdigest(), name))
    return SO


def lib():
    global _lib
    if _lib is None:
        if not available():
            raise RuntimeError(SO + " is missing: run __graft_entry__.build() where the reference is present")
        _lib = ctypes.CDLL(SO)
        for s in SYMBOLS:
            getattr(_lib, s).restype = None
    return _lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t):
    import torch
    assert t.is_cuda and t.dtype == torch.float32
    return t.contiguous()


def _i32(t, bound):
    import torch
    assert t.is_cuda and t.dtype == torch.int32
    assert t.numel() > 0 and int(t.min()) >= 0 and int(t.max()) < bound, "index outside the gathered dimension"
    return t.contiguous()


def _nonzero(*dims):
    assert all(int(d) >= 1 for d in dims), "the reference's launch configuration is undefined for a zero size"


def furthest_point_sampling(xyz, m):
    import torch
    xyz = _f32(xyz)
    b, n, _ = xyz.shape
    _nonzero(b, n, m)
    temp = torch.full((b, n), 1e10, dtype=torch.float32, device=xyz.device)
    out = torch.zeros((b, m), dtype=torch.int32, device=xyz.device)
    lib().pn2ref_furthest_point_sampling(b, n, int(m), _p(xyz), _p(temp), _p(out), _stream())
    return out


def gather_points(points, idx):
    import torch
    points = _f32(points)
    b, c, n = points.shape
    idx = _i32(idx, n)
    m = idx.shape[1]
    _nonzero(b, c, n, m)
    out = torch.zeros((b, c, m), dtype=torch.float32, device=points.device)
    lib().pn2ref_gather_points(b, c, n, m, _p(points), _p(idx), _p(out), _stream())
    return out


def gather_points_grad(grad_out, idx, n):
    import torch
    grad_out = _f32(grad_out)
    b, c, m = grad_out.shape
    idx = _i32(idx, n)
    _nonzero(b, c, n, m)
    out = torch.zeros((b, c, int(n)), dtype=torch.float32, device=grad_out.device)
    lib().pn2ref_gather_points_grad(b, c, int(n), m, _p(grad_out), _p(idx), _p(out), _stream())
    return out


def ball_query(new_xyz, xyz, radius, nsample):
    import torch
    new_xyz, xyz = _f32(new_xyz), _f32(xyz)
    b, m, _ = new_xyz.shape
    n = xyz.shape[1]
    _nonzero(b, m, n, nsample)
    out = torch.zeros((b, m, int(nsample)), dtype=torch.int32, device=xyz.device)
    lib().pn2ref_ball_query(b, n, m, ctypes.c_float(radius), int(nsample), _p(new_xyz), _p(xyz), _p(out), _stream())
    return out


def group_points(points, idx):
    import torch
    points = _f32(points)
    b, c, n = points.shape
    idx = _i32(idx, n)
    _, npoints, nsample = idx.shape
    _nonzero(b, c, n, npoints, nsample)
    out = torch.zeros((b, c, npoints, nsample), dtype=torch.float32, device=points.device)
    lib().pn2ref_group_points(b, c, n, npoints, nsample, _p(points), _p(idx), _p(out), _stream())
    return out


def group_points_grad(grad_out, idx, n):
    import torch
    grad_out = _f32(grad_out)
    b, c, npoints, nsample = grad_out.shape
    idx = _i32(idx, n)
    _nonzero(b, c, n, npoints, nsample)
    out = torch.zeros((b, c, int(n)), dtype=torch.float32, device=grad_out.device)
    lib().pn2ref_group_points_grad(b, c, int(n), npoints, nsample, _p(grad_out), _p(idx), _p(out), _stream())
    return out


def three_nn(unknown, known):
    import torch
    unknown, known = _f32(unknown), _f32(known)
    b, n, _ = unknown.shape
    m = known.shape[1]
    _nonzero(b, n, m)
    dist2 = torch.zeros((b, n, 3), dtype=torch.float32, device=unknown.device)
    idx = torch.zeros((b, n, 3), dtype=torch.int32, device=unknown.device)
    lib().pn2ref_three_nn(b, n, m, _p(unknown), _p(known), _p(dist2), _p(idx), _stream())
    return dist2, idx


def three_interpolate(points, idx, weight):
    import torch
    points, weight = _f32(points), _f32(weight)
    b, c, m = points.shape
    idx = _i32(idx, m)
    n = idx.shape[1]
    _nonzero(b, c, m, n)
    out = torch.zeros((b, c, n), dtype=torch.float32, device=points.device)
    lib().pn2ref_three_interpolate(b, c, m, n, _p(points), _p(idx), _p(weight), _p(out), _stream())
    return out


def three_interpolate_grad(grad_out, idx, weight, m):
    import torch
    grad_out, weight = _f32(grad_out), _f32(weight)
    b, c, n = grad_out.shape
    idx = _i32(idx, m)
    _nonzero(b, c, n, m)
    out = torch.zeros((b, c, int(m)), dtype=torch.float32, device=grad_out.device)
    lib().pn2ref_three_interpolate_grad(b, c, n, int(m), _p(grad_out), _p(idx), _p(weight), _p(out), _stream())
    return out
