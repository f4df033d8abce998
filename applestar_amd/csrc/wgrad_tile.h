// What the fp32 weight-gradient kernels (wgrad_f32.hip, conv_wgrad_f32_halo.hip) share: the decode of a workgroup
// into its dW tile and row slice, and the walk of reduction rows over NHWC images - the one place that decides
// whether a neighbouring image's pixels can enter a gradient (the weight-gradient side of conv_tap.h).
#pragma once
#include "common.h"

namespace as {

// workgroup wg (after xcd_remap) of a grid of tiles_k x tiles_n x S: K tile fastest, then N tile, then row slice s
struct WgTile {
  int tk, tn, s, n0, k0;
  long r_begin, r_end;
};

template <int BN, int BK>
__device__ __forceinline__ WgTile wg_tile(int wg, int tiles_n, int tiles_k, long rows_per_split, long R) {
  WgTile t;
  t.tk = wg % tiles_k;
  t.tn = (wg / tiles_k) % tiles_n;
  t.s = wg / (tiles_k * tiles_n);
  t.n0 = t.tn * BN;
  t.k0 = t.tk * BK;
  t.r_begin = static_cast<long>(t.s) * rows_per_split;
  t.r_end = t.r_begin + rows_per_split < R ? t.r_begin + rows_per_split : R;
  return t;
}

// image coordinates of a reduction row (pixel) of [B, H, W] images, walked forward without divisions
struct ImageCursor {
  int y, x;
  __device__ __forceinline__ void init(long row, long HW, int W) {
    const int rem = static_cast<int>(row % HW);
    y = rem / W;
    x = rem - y * W;
  }
  // `rows` >= 0 pixels as a displacement (whole image rows, rest): loop-invariant, so taken once per kernel
  static __device__ __forceinline__ ImageCursor stride(int rows, int W) { return ImageCursor{rows / W, rows % W}; }
  // move on by stride(rows, W); a step may pass over several images (rows / W >= H)
  __device__ __forceinline__ void advance(const ImageCursor by, int H, int W) {
    x += by.x;
    y += by.y;
    if (x >= W) { x -= W; ++y; }
    while (y >= H) y -= H;
  }
};

// A lane's fixed 16-B piece of the X operand of the implicit im2col (k = tap Cin + c): channels c .. c + 3 of the
// pixel shifted by the tap (dy, dx) of column b_col.  Dense X ([R, K]): c = b_col, no shift.
template <bool CONV>
struct WgConvPiece {
  int c, dy, dx;
  __device__ __forceinline__ void init(int b_col, int Cin) {
    c = b_col;
    dy = dx = 0;
    if (CONV) {
      const int tap = b_col / Cin;
      c = b_col - tap * Cin;
      dy = tap / 3 - 1;
      dx = tap % 3 - 1;
    }
  }
  // byte offset of the piece for reduction row (pixel) r
  __device__ __forceinline__ int offset(int r, int W, int Cin) const { return ((r + dy * W + dx) * Cin + c) * 4; }
};

}  // namespace as
