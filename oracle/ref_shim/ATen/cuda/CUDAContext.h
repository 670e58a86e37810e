/* oracle/ref_shim/ATen/cuda/CUDAContext.h -- stand-in: the "current stream" the reference's launch wrappers
 * ask for is a settable global, written by every pn2ref_* entry point (oracle/pn2_ref_glue.cpp) before it
 * calls the wrapper. */
#pragma once
#include <hip/hip_runtime.h>

extern "C" hipStream_t pn2ref_current_stream;

namespace at {
namespace cuda {
inline hipStream_t getCurrentCUDAStream() { return pn2ref_current_stream; }
}  // namespace cuda
}  // namespace at
