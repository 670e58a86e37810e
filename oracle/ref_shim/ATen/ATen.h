/* oracle/ref_shim/ATen/ATen.h -- stand-in: the reference's device files include ATen but use none of it
 * beyond the current stream (ATen/cuda/CUDAContext.h beside this file). */
#pragma once
