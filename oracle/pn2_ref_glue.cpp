/*
 * oracle/pn2_ref_glue.cpp -- C entry points into the reference's own pointnet2 launch wrappers.
 *
 * TEST INFRASTRUCTURE ONLY.  oracle/pn2_ref.py compiles the reference's four device files, unmodified and
 * from where the reference lies, together with this file into oracle/_ref/libpn2_ref.so; nothing of the
 * reference is part of this tree.  This file only names the nine wrappers (their prototypes as the reference's
 * host files declare them), sets the stream the stand-in at::cuda::getCurrentCUDAStream() returns, and calls
 * them on device pointers.  Allocation and initialisation of outputs (temp = 1e10, zeroed outputs and
 * gradients) is the caller's job, as it is the job of the reference's host files.
 */
#include <hip/hip_runtime.h>

extern "C" {
hipStream_t pn2ref_current_stream = nullptr;
}

void furthest_point_sampling_kernel_wrapper(int b, int n, int m, const float *dataset, float *temp, int *idxs);
void gather_points_kernel_wrapper(int b, int c, int n, int npoints, const float *points, const int *idx,
                                  float *out);
void gather_points_grad_kernel_wrapper(int b, int c, int n, int npoints, const float *grad_out, const int *idx,
                                       float *grad_points);
void query_ball_point_kernel_wrapper(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                                     const float *xyz, int *idx);
void group_points_kernel_wrapper(int b, int c, int n, int npoints, int nsample, const float *points,
                                 const int *idx, float *out);
void group_points_grad_kernel_wrapper(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                                      const int *idx, float *grad_points);
void three_nn_kernel_wrapper(int b, int n, int m, const float *unknown, const float *known, float *dist2,
                             int *idx);
void three_interpolate_kernel_wrapper(int b, int c, int m, int n, const float *points, const int *idx,
                                      const float *weight, float *out);
void three_interpolate_grad_kernel_wrapper(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                           const float *weight, float *grad_points);

static inline void use(void *stream) { pn2ref_current_stream = static_cast<hipStream_t>(stream); }

extern "C" {

void pn2ref_furthest_point_sampling(int b, int n, int m, const float *dataset, float *temp, int *idxs,
                                    void *stream) {
  use(stream);
  furthest_point_sampling_kernel_wrapper(b, n, m, dataset, temp, idxs);
}

void pn2ref_gather_points(int b, int c, int n, int npoints, const float *points, const int *idx, float *out,
                          void *stream) {
  use(stream);
  gather_points_kernel_wrapper(b, c, n, npoints, points, idx, out);
}

void pn2ref_gather_points_grad(int b, int c, int n, int npoints, const float *grad_out, const int *idx,
                               float *grad_points, void *stream) {
  use(stream);
  gather_points_grad_kernel_wrapper(b, c, n, npoints, grad_out, idx, grad_points);
}

void pn2ref_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz,
                       int *idx, void *stream) {
  use(stream);
  query_ball_point_kernel_wrapper(b, n, m, radius, nsample, new_xyz, xyz, idx);
}

void pn2ref_group_points(int b, int c, int n, int npoints, int nsample, const float *points, const int *idx,
                         float *out, void *stream) {
  use(stream);
  group_points_kernel_wrapper(b, c, n, npoints, nsample, points, idx, out);
}

void pn2ref_group_points_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                              const int *idx, float *grad_points, void *stream) {
  use(stream);
  group_points_grad_kernel_wrapper(b, c, n, npoints, nsample, grad_out, idx, grad_points);
}

void pn2ref_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx,
                     void *stream) {
  use(stream);
  three_nn_kernel_wrapper(b, n, m, unknown, known, dist2, idx);
}

void pn2ref_three_interpolate(int b, int c, int m, int n, const float *points, const int *idx,
                              const float *weight, float *out, void *stream) {
  use(stream);
  three_interpolate_kernel_wrapper(b, c, m, n, points, idx, weight, out);
}

void pn2ref_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                   const float *weight, float *grad_points, void *stream) {
  use(stream);
  three_interpolate_grad_kernel_wrapper(b, c, n, m, grad_out, idx, weight, grad_points);
}

}  // extern "C"
