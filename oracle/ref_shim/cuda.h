/* oracle/ref_shim/cuda.h -- stand-in for the CUDA driver header when the reference's pointnet2 device files
 * are compiled as HIP for the cross-check library (oracle/pn2_ref.py).  Everything they use comes from
 * cuda_runtime.h beside this file. */
#pragma once
