// Weight (and bias) gradient of the 3 x 3 / pad 1 convolution, fp32 operands, fp32-accurate bf16x6 split MFMAs
// (split_mfma.h), halo-window design: the weight-gradient counterpart of conv3x3_f32_halo.hip.
//
//   dW[n, tap, c] = sum_p dY[p, n] X[p + dy W + dx, c]  (zero where the tap leaves p's image)     db[n] = sum_p dY[p, n]
//
// The kernels of wgrad_f32.hip run this as an implicit im2col over K = 9 Cin, one workgroup per (tap, row slice):
// every dY element and every input pixel of a slice goes L2 -> LDS and through the fp32 -> 3 x bf16 split nine
// times.  Here a workgroup owns ALL NINE taps of a chunk of 32 input channels for 128 outputs and one row slice
// (a 128 x 288 tile of dW):
//
//   * per stage of 16 reduction rows (pixels) it loads the dY rows [16][128] once and splits them once (split4)
//     into three bf16 planes, double-buffered;
//   * the input is a window of the stage's pixels plus one image row and one pixel of halo on each side, held as
//     three bf16 planes in a ring of NRING pixel rows: the window advances by the stage's 16 rows (16 new rows
//     are loaded and split per stage, once), it is never reloaded;
//   * both kinds of plane are stored in natural [pixel][channel] order and the MFMA fragments - 8 consecutive
//     pixels of one column per lane: the pixel is the reduction index - are read with the transposing
//     ds_read_b64_tr_b16 (two per plane and fragment).  A tap is a row offset of the read.  dY and X fragments
//     are read with the same lane -> pixel map, so the order of the 16 pixels inside an MFMA does not matter;
//   * in the transposing read each lane supplies the address of ONE pixel row (lane 4 q + p of a 16-lane group:
//     row q, columns 4 p .. 4 p + 3), so the image edges are handled per reduction row: a lane whose pixel's tap
//     leaves the image points at a zero row instead (never a multiplication by a mask: a NaN in the neighbouring
//     image cannot leak).  The read needs EXEC all ones: no lane-dependent control flow in the stage loop.
//
// Waves: four along the outputs; each holds 9 (taps) 32 x 32 accumulators (144 registers) and per stage reads one
// dY fragment and nine X fragments for 54 MFMAs.  Per stage a thread splits 8 dY floats and at most 4 X floats:
// under 2 split VALU per MFMA against ~6 in the per-tap kernels.  The dY planes' row pitch is 64 B past a multiple of
// 256 B and the X planes' exactly 64 B, so the four pixel rows x 64 B a half-wave reads cover all 64 banks once.
//
// Partials: slice s writes [N][9 Cin] (k = tap Cin + c) at dw_part + s part_stride and, from the chunk-0
// workgroups, db at db_part + s part_stride: the layout of wgrad_f32.hip, whose slices (wgrad_f32_splits) it
// takes as they are - for the outputs it covers that count is set by the 64 MB bound on the partials, not by the
// number of tiles.  Summation order: fixed (stage by stage, no atomics); a stage holds the same 16 rows as in the
// split-once kernel of wgrad_f32.hip and db is summed in that kernel's order, so both results have its bits.
//
// At most 64 outputs cannot fill four waves along the outputs: conv_wgrad_f32_halo_narrow_kernel below puts the
// waves along the reduction rows instead (its budget and order are written there) and has its own slice count.
//
// This file: the two kernels, their launchers, the support predicate, the slice count of a conv
// (conv_wgrad_f32_splits) and the switch (conv_wgrad_halo_f32_mode).
#include <cstdlib>

#include "../common.h"
#include "../kernels.h"
#include "../split_mfma.h"
#include "../f32_pipe.h"
#include "../conv_tap.h"

namespace as {
namespace {

using pipe::f16v;

constexpr int kWgBN = 128, kWgCC = 32, kWgRS = 16, kWgMaxW = 80;

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

template <int WMAX>
struct WgHaloCfg {
  static constexpr int SA = kWgBN * 2 + 64, SX = kWgCC * 2;                     // plane row pitches (bytes)
  static constexpr int NRING = 2 * kWgRS + 2 * WMAX + 2 <= 128 ? 128 : 256;     // window + the incoming stage's rows
  static constexpr int PA = kWgRS * SA;                                         // one dY plane of one stage
  static constexpr int PX = (NRING + 1) * SX;                                   // one X plane + the zero row
  static constexpr int SMEM = 6 * PA + 3 * PX;
  static_assert(2 * kWgRS + 2 * WMAX + 2 <= NRING && 2 * SMEM <= 160 * 1024, "ring size / two workgroups per CU");
};

// 4 pixel rows x 16 columns of bf16 per 16-lane group, delivered column-major (this lane: its group's column
// lane & 15, the four rows)
__device__ __forceinline__ s16x4 tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
}

__device__ __forceinline__ u32v4 tr_frag(const char* p0, const char* p1) {
  const uint2 lo = __builtin_bit_cast(uint2, tr_read(p0)), hi = __builtin_bit_cast(uint2, tr_read(p1));
  return u32v4{lo.x, lo.y, hi.x, hi.y};
}

__device__ __forceinline__ void split_store(char* plane0, int plane_bytes, int off, const uint4 v) {
  uint2 s0, s1, s2;
  split4(v, s0, s1, s2);
  *reinterpret_cast<uint2*>(plane0 + off) = s0;
  *reinterpret_cast<uint2*>(plane0 + plane_bytes + off) = s1;
  *reinterpret_cast<uint2*>(plane0 + 2 * plane_bytes + off) = s2;
}

template <int WMAX>
__global__ __launch_bounds__(256, 2) void conv_wgrad_f32_halo_kernel(const float* __restrict__ dy,
                                                                     const float* __restrict__ x,
                                                                     float* __restrict__ dw_part,
                                                                     float* __restrict__ db_part, long part_stride,
                                                                     long R, int N, int K, int H, int W, int Cin,
                                                                     long rows_per_split, int tiles_n, int chunks) {
  using C = WgHaloCfg<WMAX>;
  constexpr int RS = kWgRS, BN = kWgBN, CC = kWgCC, SA = C::SA, SX = C::SX;
  constexpr int RINGB = C::NRING * SX;            // ring bytes per plane (a power of two); the zero row follows
  __shared__ __attribute__((aligned(16))) char smem[C::SMEM];
  char* const pa = smem;               // dY planes [buffer 2][plane 3][RS][SA]
  char* const px = smem + 6 * C::PA;   // X planes [plane 3][NRING + 1][SX]; row NRING is the zero row

  const int wg = pipe::xcd_remap();
  const int ch = wg % chunks;
  const int tn = (wg / chunks) % tiles_n;
  const int s = wg / (chunks * tiles_n);
  const int n0 = tn * BN, c0 = ch * CC;
  const long r_begin = static_cast<long>(s) * rows_per_split;
  const long r_end = r_begin + rows_per_split < R ? r_begin + rows_per_split : R;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, h = lane >> 5;
  const int HW = H * W;
  const __amdgpu_buffer_rsrc_t yr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy), 0, static_cast<int>(R * N * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, static_cast<int>(R * Cin * 4), 0x00020000);
  const int nrows = r_end > r_begin ? static_cast<int>(r_end - r_begin) : 0;
  const int nsteps = (nrows + RS - 1) / RS;

  // ---- staging: piece = (row of the stage, 4 consecutive columns); global fp32 -> registers -> split -> planes.
  // Stage j's piece is at byte offset base + j step while j RS < lim (rows left for that piece), else zeros
  // dY: two pieces per thread, rows tid / 32 and + 8, columns n0 + 4 (tid % 32) ..
  const int a_q = tid & 31, a_row = tid >> 5;
  const bool a_colok = n0 + 4 * a_q < N;
  int a_base[2], a_lim[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    a_base[i] = static_cast<int>(((r_begin + a_row + 8 * i) * N + n0 + 4 * a_q) * 4);
    a_lim[i] = a_colok ? nrows - (a_row + 8 * i) : 0;
  }
  const int a_step = RS * N * 4;
  // X: the RS rows that complete stage j's window (j >= 1) are pixels r_begin + j RS + W + 1 + row; one piece for
  // each thread of waves 0 and 1: row tid / 8, channels c0 + 4 (tid % 8) ..
  const int x_q = tid & 7, x_row = (tid >> 3) & 15;
  const bool x_colok = c0 + 4 * x_q < Cin, x_wave = wid < 2;
  const int x_base = static_cast<int>(((r_begin + W + 1 + x_row) * Cin + c0 + 4 * x_q) * 4);
  const long x_left = R - (r_begin + W + 1 + x_row);
  const int x_lim = (x_colok && x_wave && x_left > 0) ? static_cast<int>(x_left) : 0;
  const int x_step = RS * Cin * 4;
  // db (chunk-0 workgroups): the column sums in the order of wgrad_f32.hip's split-once kernel, so db comes out
  // bit for bit as there - thread (column tid % 128, half tid / 128) adds rows 8 half .. + 7 of every stage to one
  // running sum, and the two halves are added at the end.  The rows are re-read from L2 as single floats: the
  // pieces above hold four columns of two rows, the wrong shape for that order
  const bool do_bias = db_part != nullptr && ch == 0;
  const int b_col = n0 + (tid & 127), b_h = tid >> 7;
  const int b_base = static_cast<int>(((r_begin + 8 * b_h) * N + b_col) * 4);
  const int b_lim = b_col < N ? nrows - 8 * b_h : 0;
  float rb[8], bsum = 0.f;
  uint4 ra[2], rx;
  auto load_stage = [&](int j) {
    if (do_bias) {
#pragma unroll
      for (int q = 0; q < 8; ++q)
        rb[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
            yr, j * RS + q < b_lim ? b_base + j * a_step + q * N * 4 : kOOB, 0, 0));
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const auto v =
          __builtin_amdgcn_raw_buffer_load_b128(yr, j * RS < a_lim[i] ? a_base[i] + j * a_step : kOOB, 0, 0);
      ra[i] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(xr, j * RS < x_lim ? x_base + j * x_step : kOOB, 0, 0);
    rx = make_uint4(v[0], v[1], v[2], v[3]);
  };
  auto add_bias = [&]() {
    if (do_bias) {
#pragma unroll
      for (int q = 0; q < 8; ++q) bsum += rb[q];
    }
  };
  const int a_dst = a_row * SA + a_q * 8;
  const int x_dst0 = (2 * (W + 1) + x_row) * SX + x_q * 8;      // + j RS SX, modulo the ring: pixel - (r_begin - (W + 1))
  auto store_stage = [&](int j) {
#pragma unroll
    for (int i = 0; i < 2; ++i) split_store(pa + (j & 1) * 3 * C::PA, C::PA, a_dst + 8 * i * SA, ra[i]);
    add_bias();
    if (x_wave) split_store(px, C::PX, (x_dst0 + j * RS * SX) & (RINGB - 1), rx);     // wave-uniform
  };

  // ---- fragment addressing: lane = group g (16 lanes) x (row q, column quad p) of the transposing read
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  const int rr0 = 8 * (g >> 1) + tq;                            // this lane's pixel rows of a stage: rr0, rr0 + 4
  const int a_off = rr0 * SA + (32 * wid + 16 * (g & 1) + 4 * tp) * 2;
  const int x_col = (16 * (g & 1) + 4 * tp) * 2;                // < SX: the byte within a ring row
  const int x_off0 = (W + 1 + rr0) * SX + x_col;                // + j RS SX + the tap's shift, modulo the ring
  const int x_zero = RINGB + x_col;
  int shb[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) shb[t] = ((t / 3 - 1) * W + (t % 3 - 1)) * SX;
  // image coordinates of the lane's two pixels of the next stage to compute, advanced by RS pixels per stage
  int py[2], pxx[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int rem = static_cast<int>((r_begin + rr0 + 4 * r) % HW);
    py[r] = rem / W;
    pxx[r] = rem - py[r] * W;
  }
  const int adv = RS % HW, adv_y = adv / W, adv_x = adv - adv_y * W;

  f16v acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  // ---- prologue: the zero row, stage 0's window (RS + 2 W + 2 rows from pixel r_begin - (W + 1)) and dY rows
  for (int i = tid; i < 3 * SX / 4; i += 256)
    *reinterpret_cast<unsigned*>(px + (i / (SX / 4)) * C::PX + RINGB + (i % (SX / 4)) * 4) = 0u;
  load_stage(0);
  {
    const int npieces = (RS + 2 * W + 2) * (CC / 4);
    for (int piece = tid; piece < npieces; piece += 256) {
      const int row = piece >> 3;
      const long pix = r_begin - (W + 1) + row;
      const bool ok = x_colok && pix >= 0 && pix < R;
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(
          xr, ok ? (static_cast<int>(pix) * Cin + c0 + 4 * x_q) * 4 : kOOB, 0, 0);
      split_store(px, C::PX, row * SX + x_q * 8, make_uint4(v[0], v[1], v[2], v[3]));
    }
  }
  {
    // stage 0's dY only: its window rows came from the loop above
#pragma unroll
    for (int i = 0; i < 2; ++i) split_store(pa, C::PA, a_dst + 8 * i * SA, ra[i]);
    add_bias();
  }
  __syncthreads();

  for (int j = 0; j < nsteps; ++j) {
    const bool more = j + 1 < nsteps;
    if (more) load_stage(j + 1);
    // per-tap validity (9 bits) of the lane's two pixels, then their coordinates for the next stage
    int ok[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      ok[r] = conv_tap_mask_yx(py[r], pxx[r], H, W);
      pxx[r] += adv_x;
      py[r] += adv_y;
      if (pxx[r] >= W) { pxx[r] -= W; ++py[r]; }
      if (py[r] >= H) py[r] -= H;
    }
    const char* ap = pa + (j & 1) * 3 * C::PA + a_off;
    Split3 fa;
#pragma unroll
    for (int p = 0; p < 3; ++p) fa.p[p] = tr_frag(ap + p * C::PA, ap + p * C::PA + 4 * SA);
    const int xs = x_off0 + j * RS * SX;                        // ring byte (before the wrap) of the lane's first pixel
    auto read_x = [&](int t) {
      // in the image: the ring row of pixel + shift; else the zero row (select by the tap's bit spread to a mask)
      const int m0 = __builtin_amdgcn_sbfe(ok[0], t, 1), m1 = __builtin_amdgcn_sbfe(ok[1], t, 1);
      const int o0 = (((xs + shb[t]) & (RINGB - 1)) & m0) | (x_zero & ~m0);
      const int o1 = (((xs + 4 * SX + shb[t]) & (RINGB - 1)) & m1) | (x_zero & ~m1);
      Split3 f;
#pragma unroll
      for (int p = 0; p < 3; ++p) f.p[p] = tr_frag(px + p * C::PX + o0, px + p * C::PX + o1);
      return f;
    };
    // tap t + 1's fragments are read before tap t's MFMAs issue: the LDS latency hides behind the six products
    Split3 fb[2];
    fb[0] = read_x(0);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      if (t + 1 < 9) fb[(t + 1) & 1] = read_x(t + 1);
      __builtin_amdgcn_sched_barrier(0);                        // left alone the scheduler sinks the reads again
      acc[t] = mfma_x6(fa, fb[t & 1], acc[t]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) store_stage(j + 1);
    __syncthreads();
  }

  // accumulator t register e: n = n0 + 32 wave + (e & 3) + 8 (e >> 2) + 4 h, k = t Cin + c0 + l32
  float* outp = dw_part + static_cast<long>(s) * part_stride;
  const int c = c0 + l32;
  if (c < Cin) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = n0 + 32 * wid + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (n < N) outp[static_cast<long>(n) * K + t * Cin + c] = acc[t][e];
      }
  }
  if (do_bias) {
    float* red = reinterpret_cast<float*>(smem);                // the planes are idle (barrier above)
    red[tid] = bsum;
    __syncthreads();
    if (b_h == 0 && b_col < N) db_part[static_cast<long>(s) * part_stride + b_col] = bsum + red[tid + 128];
  }
}

template <int WMAX>
void launch_wg_halo(const float* dy, const float* x, float* dwp, float* dbp, long ps, long R, int N, int K, int H,
                    int W, int Cin, int S, long rps, hipStream_t st) {
  const int tiles_n = (N + kWgBN - 1) / kWgBN, chunks = (Cin + kWgCC - 1) / kWgCC;
  const long nwg = static_cast<long>(S) * tiles_n * chunks;
  hipLaunchKernelGGL((conv_wgrad_f32_halo_kernel<WMAX>), dim3(static_cast<unsigned>(nwg)), dim3(256), 0, st, dy, x,
                     dwp, dbp, ps, R, N, K, H, W, Cin, rps, tiles_n, chunks);
}

// ---- at most 64 outputs: the waves along the reduction rows -------------------------------------------------
// WN = 1 (N <= 32) or 2 (N <= 64) waves along the outputs, WR = 4 / WN along the rows of a stage of RS = 16 WR
// pixels: wave (wn, wr) multiplies rows 16 wr .. + 15 of every stage into its own nine 32 x 32 accumulators for
// outputs 32 wn .., so per stage and wave the work is that of the kernel above (one dY fragment, nine X fragments,
// 54 MFMAs) and a workgroup again owns all nine taps of a 32-channel chunk - of all outputs.  At the end of the
// slice the WR copies are added through the LDS in the order wr = 0, 1, .. (no atomics: the order is fixed).
// A stage of 64 rows with the incoming stage beside the window would need a ring of 2 RS + 2 W + 2 = 290 rows at
// W = 80, i.e. 512: 98 KB.  So nothing is double-buffered here: the next stage's rows are stored after a second
// barrier, over the rows the window has just left (ring >= RS + 2 W + 2 = 226 -> 256 rows); its global loads are
// still issued before the stage's MFMAs.  Two barriers per 64 or 32 rows are no more than the one per 16 above.
//   LDS   WN = 1: dY 3 x 64 x 64 B = 12.0 KB, X 3 x 257 x 64 B = 48.2 KB: 60.2 KB
//         WN = 2: dY 3 x 32 x 192 B = 18.0 KB, X 48.2 KB: 66.2 KB            (two workgroups per CU: <= 80 KB)
//   VGPR  144 accumulators + 36 fragments (dY, two taps of X) + 16 staged floats + addressing: 2 waves per SIMD
// -Rpass-analysis=kernel-resource-usage: WN = 1 238 VGPRs, 61,632 B of LDS; WN = 2 232 VGPRs, 67,776 B; no AGPRs,
// no scratch, 2 waves per SIMD (the kernel above: 245 VGPRs, 55,488 / 80,064 B).  db: every thread adds the dY pieces it stages (4
// columns of 2 rows per stage) to four running sums; the threads of a column are added through the LDS in thread
// order at the end.  A half-empty tile (16 outputs, 16 channels) runs its MFMAs on zeros.
template <int WN>
struct WgNarrowCfg {
  static constexpr int WR = 4 / WN, RS = 16 * WR, BN = 32 * WN;
  static constexpr int SA = BN == 32 ? 64 : BN * 2 + 64, SX = kWgCC * 2;         // four rows cover all 64 banks once
  static constexpr int NRING = 256;
  static constexpr int PA = RS * SA, PX = (NRING + 1) * SX;
  static constexpr int SMEM = 3 * PA + 3 * PX;
  static constexpr int TH = 5;                                                  // taps per pass of the final sum
  static_assert(RS + 2 * kWgMaxW + 2 <= NRING && 2 * SMEM <= 160 * 1024, "ring size / two workgroups per CU");
  static_assert(WN * TH * 16 * 64 * 4 <= SMEM && 256 * 4 * 4 <= SMEM, "the final sums reuse the planes");
};

template <int WN>
__global__ __launch_bounds__(256, 2) void conv_wgrad_f32_halo_narrow_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dw_part,
    float* __restrict__ db_part, long part_stride, long R, int N, int K, int H, int W, int Cin, long rows_per_split,
    int chunks) {
  using C = WgNarrowCfg<WN>;
  constexpr int RS = C::RS, BN = C::BN, CC = kWgCC, SA = C::SA, SX = C::SX, WR = C::WR;
  constexpr int RINGB = C::NRING * SX;
  constexpr int AQ = BN / 4, AROWS = 256 / AQ;    // dY pieces: AQ column quads per row, AROWS rows per pass, 2 passes
  constexpr int XP = RS / 32;                     // X pieces per thread: 8 quads per row, 32 rows per pass
  static_assert(2 * AROWS == RS, "two dY pieces per thread");
  __shared__ __attribute__((aligned(16))) char smem[C::SMEM];
  char* const pa = smem;               // dY planes [plane 3][RS][SA]
  char* const px = smem + 3 * C::PA;   // X planes [plane 3][NRING + 1][SX]; row NRING is the zero row

  const int wg = pipe::xcd_remap();
  const int ch = wg % chunks;
  const int s = wg / chunks;
  const int c0 = ch * CC;
  const long r_begin = static_cast<long>(s) * rows_per_split;
  const long r_end = r_begin + rows_per_split < R ? r_begin + rows_per_split : R;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wid % WN, wr = wid / WN;
  const int l32 = lane & 31, h = lane >> 5;
  const int HW = H * W;
  const __amdgpu_buffer_rsrc_t yr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy), 0, static_cast<int>(R * N * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, static_cast<int>(R * Cin * 4), 0x00020000);
  const int nrows = r_end > r_begin ? static_cast<int>(r_end - r_begin) : 0;
  const int nsteps = (nrows + RS - 1) / RS;

  // ---- staging, as above: piece = (row of the stage, 4 consecutive columns)
  const int a_q = tid % AQ, a_row = tid / AQ;
  const bool a_colok = 4 * a_q < N;
  int a_base[2], a_lim[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    a_base[i] = static_cast<int>(((r_begin + a_row + AROWS * i) * N + 4 * a_q) * 4);
    a_lim[i] = a_colok ? nrows - (a_row + AROWS * i) : 0;
  }
  const int a_step = RS * N * 4;
  const int x_q = tid & 7, x_row = tid >> 3;
  const bool x_colok = c0 + 4 * x_q < Cin;
  int x_base[XP], x_lim[XP];
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const long pix = r_begin + W + 1 + x_row + 32 * i;
    x_base[i] = static_cast<int>((pix * Cin + c0 + 4 * x_q) * 4);
    x_lim[i] = (x_colok && R - pix > 0) ? static_cast<int>(R - pix) : 0;
  }
  const int x_step = RS * Cin * 4;
  const bool do_bias = db_part != nullptr && ch == 0;
  float bs[4] = {0.f, 0.f, 0.f, 0.f};
  uint4 ra[2], rx[XP];
  auto load_stage = [&](int j) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const auto v =
          __builtin_amdgcn_raw_buffer_load_b128(yr, j * RS < a_lim[i] ? a_base[i] + j * a_step : kOOB, 0, 0);
      ra[i] = make_uint4(v[0], v[1], v[2], v[3]);
    }
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      const auto v =
          __builtin_amdgcn_raw_buffer_load_b128(xr, j * RS < x_lim[i] ? x_base[i] + j * x_step : kOOB, 0, 0);
      rx[i] = make_uint4(v[0], v[1], v[2], v[3]);
    }
  };
  const int a_dst = a_row * SA + a_q * 8;
  auto store_a = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      split_store(pa, C::PA, a_dst + AROWS * i * SA, ra[i]);
      bs[0] += __uint_as_float(ra[i].x);
      bs[1] += __uint_as_float(ra[i].y);
      bs[2] += __uint_as_float(ra[i].z);
      bs[3] += __uint_as_float(ra[i].w);
    }
  };
  const int x_dst0 = (2 * (W + 1) + x_row) * SX + x_q * 8;      // + j RS SX, modulo the ring
  auto store_stage = [&](int j) {
    store_a();
#pragma unroll
    for (int i = 0; i < XP; ++i) split_store(px, C::PX, (x_dst0 + (j * RS + 32 * i) * SX) & (RINGB - 1), rx[i]);
  };

  // ---- fragment addressing, as above; the wave's rows of a stage start at 16 wr
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  const int rr0 = 16 * wr + 8 * (g >> 1) + tq;
  const int a_off = rr0 * SA + (32 * wn + 16 * (g & 1) + 4 * tp) * 2;
  const int x_col = (16 * (g & 1) + 4 * tp) * 2;
  const int x_off0 = (W + 1 + rr0) * SX + x_col;
  const int x_zero = RINGB + x_col;
  int shb[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) shb[t] = ((t / 3 - 1) * W + (t % 3 - 1)) * SX;
  int py[2], pxx[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int rem = static_cast<int>((r_begin + rr0 + 4 * r) % HW);
    py[r] = rem / W;
    pxx[r] = rem - py[r] * W;
  }
  const int adv = RS % HW, adv_y = adv / W, adv_x = adv - adv_y * W;

  f16v acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  // ---- prologue: the zero row, stage 0's window (RS + 2 W + 2 rows from pixel r_begin - (W + 1)) and dY rows
  for (int i = tid; i < 3 * SX / 4; i += 256)
    *reinterpret_cast<unsigned*>(px + (i / (SX / 4)) * C::PX + RINGB + (i % (SX / 4)) * 4) = 0u;
  load_stage(0);
  {
    const int npieces = (RS + 2 * W + 2) * (CC / 4);
    for (int piece = tid; piece < npieces; piece += 256) {
      const int row = piece >> 3;
      const long pix = r_begin - (W + 1) + row;
      const bool ok = x_colok && pix >= 0 && pix < R;
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(
          xr, ok ? (static_cast<int>(pix) * Cin + c0 + 4 * x_q) * 4 : kOOB, 0, 0);
      split_store(px, C::PX, row * SX + x_q * 8, make_uint4(v[0], v[1], v[2], v[3]));
    }
  }
  store_a();
  __syncthreads();

  for (int j = 0; j < nsteps; ++j) {
    const bool more = j + 1 < nsteps;
    if (more) load_stage(j + 1);
    int ok[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      ok[r] = conv_tap_mask_yx(py[r], pxx[r], H, W);
      pxx[r] += adv_x;
      py[r] += adv_y;
      if (pxx[r] >= W) { pxx[r] -= W; ++py[r]; }
      if (py[r] >= H) py[r] -= H;
    }
    const char* ap = pa + a_off;
    Split3 fa;
#pragma unroll
    for (int p = 0; p < 3; ++p) fa.p[p] = tr_frag(ap + p * C::PA, ap + p * C::PA + 4 * SA);
    const int xs = x_off0 + j * RS * SX;
    auto read_x = [&](int t) {
      const int m0 = __builtin_amdgcn_sbfe(ok[0], t, 1), m1 = __builtin_amdgcn_sbfe(ok[1], t, 1);
      const int o0 = (((xs + shb[t]) & (RINGB - 1)) & m0) | (x_zero & ~m0);
      const int o1 = (((xs + 4 * SX + shb[t]) & (RINGB - 1)) & m1) | (x_zero & ~m1);
      Split3 f;
#pragma unroll
      for (int p = 0; p < 3; ++p) f.p[p] = tr_frag(px + p * C::PX + o0, px + p * C::PX + o1);
      return f;
    };
    Split3 fb[2];
    fb[0] = read_x(0);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      if (t + 1 < 9) fb[(t + 1) & 1] = read_x(t + 1);
      __builtin_amdgcn_sched_barrier(0);
      acc[t] = mfma_x6(fa, fb[t & 1], acc[t]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) {
      __syncthreads();                                          // every wave has read stage j: its rows may go
      store_stage(j + 1);
    }
    __syncthreads();
  }

  // ---- the WR copies: wr = 1, 2, .. hand theirs to wr = 0 through the LDS (the planes are idle), TH taps a pass
  float* const red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int r = 1; r < WR; ++r)
#pragma unroll
    for (int t0 = 0; t0 < 9; t0 += C::TH) {
      if (wr == r) {
#pragma unroll
        for (int t = t0; t < t0 + C::TH && t < 9; ++t)
#pragma unroll
          for (int e = 0; e < 16; ++e) red[((wn * C::TH + t - t0) * 16 + e) * 64 + lane] = acc[t][e];
      }
      __syncthreads();
      if (wr == 0) {
#pragma unroll
        for (int t = t0; t < t0 + C::TH && t < 9; ++t)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[t][e] += red[((wn * C::TH + t - t0) * 16 + e) * 64 + lane];
      }
      __syncthreads();
    }

  // accumulator t register e: n = 32 wn + (e & 3) + 8 (e >> 2) + 4 h, k = t Cin + c0 + l32
  float* outp = dw_part + static_cast<long>(s) * part_stride;
  const int c = c0 + l32;
  if (wr == 0 && c < Cin) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = 32 * wn + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (n < N) outp[static_cast<long>(n) * K + t * Cin + c] = acc[t][e];
      }
  }
  if (do_bias) {
    // red[a_row][column]: thread tid holds columns 4 a_q .. + 3 of rows a_row, a_row + AROWS of every stage
#pragma unroll
    for (int q = 0; q < 4; ++q) red[a_row * BN + 4 * a_q + q] = bs[q];
    __syncthreads();
    if (tid < N) {
      float v = red[tid];
      for (int i = 1; i < AROWS; ++i) v += red[i * BN + tid];
      db_part[static_cast<long>(s) * part_stride + tid] = v;
    }
  }
}

template <int WN>
void launch_wg_halo_narrow(const float* dy, const float* x, float* dwp, float* dbp, long ps, long R, int N, int K,
                           int H, int W, int Cin, int S, long rps, hipStream_t st) {
  const int chunks = (Cin + kWgCC - 1) / kWgCC;
  const long nwg = static_cast<long>(S) * chunks;
  hipLaunchKernelGGL((conv_wgrad_f32_halo_narrow_kernel<WN>), dim3(static_cast<unsigned>(nwg)), dim3(256), 0, st, dy,
                     x, dwp, dbp, ps, R, N, K, H, W, Cin, rps, chunks);
}

// APPLESTAR_CONV_WGRAD_HALO_F32 / set_conv_wgrad_halo_f32_mode: bits 1 = at most 32, 2 = 33 .. 64, 4 = 128-multiples
// of outputs; 0 = the kernels of wgrad_f32.hip for every conv.  Default 7: every class passed its measurement
// (docs/PERF_LOG.md)
int& wg_halo_ref() {
  static int v = [] {
    const char* e = std::getenv("APPLESTAR_CONV_WGRAD_HALO_F32");
    return e ? std::atoi(e) & 7 : 7;
  }();
  return v;
}

// target workgroup count of the narrow classes' slices (APPLESTAR_CONV_WGRAD_HALO_WG): the resident slots, two
// per CU.  The step's six narrow shapes at 256 / 512 / 1024 / 2048: 64 -> 32 at 76 x 80 563 / 480 / 490 / 532 us,
// 32 -> 32 at 19 x 20 36 / 35 / 50 / 58 us (docs/PERF_LOG.md)
long wg_halo_narrow_target() {
  static const long v = [] {
    const char* e = std::getenv("APPLESTAR_CONV_WGRAD_HALO_WG");
    const long x = e ? std::atol(e) : 512;
    return x >= 1 ? x : 512;
  }();
  return v;
}

}  // namespace

int conv_wgrad_halo_f32_mode() { return wg_halo_ref(); }
void set_conv_wgrad_halo_f32_mode(int mode) { wg_halo_ref() = mode & 7; }

// 128-multiples of outputs: the four waves along the outputs; at most 64 (a multiple of 4): along the reduction rows
bool conv_wgrad_f32_halo_supported(int N, int H, int W, int Cin) {
  return f32_mfma_mode() == 1 && H > 0 && W > 0 && W <= kWgMaxW && Cin > 0 && Cin % 16 == 0 && N > 0 &&
         (N % 128 == 0 || (N <= 64 && N % 4 == 0));
}

bool conv_wgrad_f32_halo_selected(int N, int H, int W, int Cin) {
  const int bit = N <= 32 ? 1 : (N <= 64 ? 2 : 4);
  return (conv_wgrad_halo_f32_mode() & bit) != 0 && conv_wgrad_f32_halo_supported(N, H, W, Cin);
}

// Slices of a conv weight gradient.  The narrow classes of the halo kernel have one workgroup per slice and
// 32-channel chunk (wgrad_f32_splits counts the per-tap kernels' (32 or 64) x 128 tiles: 5 for 64 -> 32 against 2
// chunks here), so their count is the target over the chunks; a slice holds at least two stages and the partials
// stay under the 64 MB of wgrad_f32_splits.  Every other conv: wgrad_f32_splits
int conv_wgrad_f32_splits(long R, int N, int K, int H, int W, int Cin) {
  if (!(N <= 64 && conv_wgrad_f32_halo_selected(N, H, W, Cin))) return wgrad_f32_splits(R, N, K);
  const long chunks = (Cin + kWgCC - 1) / kWgCC, rs = N <= 32 ? WgNarrowCfg<1>::RS : WgNarrowCfg<2>::RS;
  long S = (wg_halo_narrow_target() + chunks - 1) / chunks;
  const long max_s = (R + 2 * rs - 1) / (2 * rs);
  if (S > max_s) S = max_s;
  const long max_part = (16L << 20) / (static_cast<long>(N) * K);
  if (S > max_part) S = max_part;
  if (S < 1) S = 1;
  return static_cast<int>(S);
}

void conv_wgrad_f32_halo(const float* dy, const float* x, float* dw_part, float* db_part, long part_stride, long R,
                         int N, int K, int H, int W, int Cin, int S, long rows_per_split, hipStream_t st) {
  if (N <= 32) launch_wg_halo_narrow<1>(dy, x, dw_part, db_part, part_stride, R, N, K, H, W, Cin, S, rows_per_split, st);
  else if (N <= 64)
    launch_wg_halo_narrow<2>(dy, x, dw_part, db_part, part_stride, R, N, K, H, W, Cin, S, rows_per_split, st);
  else if (W <= 40) launch_wg_halo<40>(dy, x, dw_part, db_part, part_stride, R, N, K, H, W, Cin, S, rows_per_split, st);
  else launch_wg_halo<kWgMaxW>(dy, x, dw_part, db_part, part_stride, R, N, K, H, W, Cin, S, rows_per_split, st);
}

}  // namespace as
