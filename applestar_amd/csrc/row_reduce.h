// Row reductions shared by the per-row loss kernels (loss.hip, sl_loss.hip): a row is held by TPR threads of a
// 256-thread workgroup - one wave (TPR == 64, four rows per workgroup) or the whole workgroup (TPR == 256).
// The TPR == 256 forms synchronise the workgroup, so every thread of it must call them.
#pragma once
#include "common.h"

namespace as {

template <int TPR>
__device__ __forceinline__ float group_max(float v, float* red) {
  v = wave_max(v);
  if constexpr (TPR == 64) {
    return v;
  } else {
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  }
}

template <int TPR>
__device__ __forceinline__ float group_sum(float v, float* red) {
  v = wave_sum(v);
  if constexpr (TPR == 64) {
    return v;
  } else {
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
  }
}

}  // namespace as
