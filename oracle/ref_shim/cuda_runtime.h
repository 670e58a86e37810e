/* oracle/ref_shim/cuda_runtime.h -- stand-in that maps the few CUDA runtime names the reference's pointnet2
 * device files use onto HIP (oracle/pn2_ref.py builds them unmodified against this directory). */
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

typedef hipStream_t cudaStream_t;
typedef hipError_t cudaError_t;
#define cudaSuccess hipSuccess
#define cudaGetLastError hipGetLastError
#define cudaGetErrorString hipGetErrorString
