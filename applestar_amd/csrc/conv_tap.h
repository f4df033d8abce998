// The implicit im2col of the 3 x 3 / pad 1 convolutions (conv3x3.hip, conv3x3_f32.hip, conv3x3_f32_v2.hip,
// conv3x3_f32_halo.hip, conv_wgrad_f32_halo.hip, gemm_f32_psb.hip): which taps of an output pixel lie inside its image, and where a
// K-step's activation piece starts.  The one place that decides whether a neighbouring image's pixels can enter a
// tile.  K = 9 Cin is tap-major: k = tap Cin + c, tap = 3 (dy + 1) + (dx + 1).
#pragma once
#include "common.h"

namespace as {

// bit t: tap t of the pixel at (yy, xx) of an H x W image reads a pixel of that image
__device__ __forceinline__ int conv_tap_mask_yx(int yy, int xx, int H, int W) {
  int ok = 0;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int y2 = yy + t / 3 - 1, x2 = xx + t % 3 - 1;
    ok |= (y2 >= 0 && y2 < H && x2 >= 0 && x2 < W) << t;
  }
  return ok;
}

// bit t: tap t of output pixel m (of M = B HW pixels, NHWC) reads a pixel of m's own image; 0 for m >= M
__device__ __forceinline__ int conv_tap_mask(long m, long M, int HW, int H, int W) {
  if (m >= M) return 0;
  const int rem = static_cast<int>(m % HW);
  const int yy = rem / W;
  return conv_tap_mask_yx(yy, rem - yy * W, H, W);
}

// the K-step that starts at k0 (inside one tap): its tap, first channel and the tap's pixel shift dy W + dx
struct ConvTap {
  int tap, c0, shift;
  __device__ __forceinline__ bool in(int mask) const { return (mask >> tap) & 1; }
  // byte offset of channel c0 + c of pixel pix shifted by the tap (elements of `es` bytes), kOOB (zeros) unless ok
  __device__ __forceinline__ int offset(bool ok, int pix, int Cin, int c, int es) const {
    return ok ? ((pix + shift) * Cin + c0 + c) * es : kOOB;
  }
};

__device__ __forceinline__ ConvTap conv_tap(int k0, int Cin, int W) {
  const int tap = k0 / Cin;
  return ConvTap{tap, k0 - tap * Cin, (tap / 3 - 1) * W + (tap % 3 - 1)};
}

}  // namespace as
