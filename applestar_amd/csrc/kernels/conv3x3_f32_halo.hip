// 3 x 3 / pad 1 convolution, fp32 operands, fp32-accurate bf16x6 split MFMAs (split_mfma.h), halo-window design:
// the fp32 form of conv3x3_halo_kernel (conv3x3.hip).
//
// The ring kernel (conv3x3_f32_v2.hip) is an implicit im2col: per (tap, 16 channels) K-step it DMAs the tile's 128
// activation rows again and every wave splits its fragment again (~44 VALU), so each input pixel goes L2 -> LDS and
// through the fp32 -> 3 x bf16 split nine times.  Here a 128-pixel tile's input is staged ONCE per 16-channel chunk
// as a window of 128 + 2 W + 2 consecutive pixel rows (the tile plus one image row and one pixel of halo on each
// side), split while it is staged (split4) into three row-major bf16 planes [row][16].  Every tap then reads its
// activation fragment from the planes at the constant row offset dy W + dx with one ds_read_b128 per plane: no
// VALU in the tap loop.  A lane whose neighbour pixel falls outside the image reads a zero slot instead (the
// per-lane, per-tap addresses are computed once per kernel; never a multiplication by a mask, so a NaN in the
// neighbouring image cannot leak).
//
// Window image: plane p = NR rows of 32 B + one 16-B zero slot; the 16-B slot of channel half c of row r is
// c ^ ((r >> 3) & 1), which puts the 16 rows of a ds_read_b128 lane group on distinct 4-bank groups at every row
// shift (lane-group model of tools/lds_bank_check.py; unswizzled rows model 2 x the cycles).
//
// Weights: the presplit_b planes, exactly as the ring kernel reads them (1 KB pieces in MFMA fragment order,
// K-step index (tap Cin + c0) / 16), LDS-DMA'd TS taps at a time into a double buffer, one barrier per stage.
// The window is single-buffered: the next chunk's pixels are loaded into registers a stage ahead and are split
// and stored after one extra barrier behind the chunk's last tap.
//
// Tile: 128 consecutive output pixels x BN (32 / 64 / 128), four waves of 32 pixels each with the transposed
// accumulator (mfma_x6(weights, activations)): pipe::store_tile and every epilogue of the ring kernel unchanged.
// The summation order per output is chunk-major (the ring's is tap-major): results differ from the ring kernel's
// in the last bits and are identical from run to run.
//
// This file: the kernel, its launcher (conv3x3_f32_halo) and what it covers (conv3x3_f32_halo_supported).  Which
// convs conv3x3_f32_psb sends here: conv3x3_f32_dispatch.hip.  The in-image tap mask: conv_tap.h.
#include "../common.h"
#include "../kernels.h"
#include "../split_mfma.h"
#include "../f32_pipe.h"
#include "../conv_tap.h"

namespace as {
namespace {

using pipe::f16v;
using pipe::i32x4;

constexpr int kHaloBM = 128, kHaloCK = 16, kHaloMaxW = 80;

// TS: taps per weight stage (1 / 3 / 9); WMAX: the widest map the window holds
template <int BN, int TS, int WMAX>
struct HaloF32Cfg {
  static constexpr int FN = BN / 32;
  static constexpr int NR = kHaloBM + 2 * WMAX + 2;        // window rows
  static constexpr int PLANE = NR * 32 + 16;               // + the zero slot
  static constexpr int WIN = 3 * PLANE;
  static constexpr int WP = (NR * 4 + 255) / 256;          // 16-B fp32 pieces per thread (4 per window row)
  static constexpr int QW = TS * FN * 3;                   // 1 KB weight pieces per stage, dealt round-robin to waves
  static constexpr int W_PW = (QW + 3) / 4;
  static constexpr int WST = QW * 1024;
  static constexpr int S = 9 / TS;                         // stages per chunk
  static constexpr int SMEM = WIN + 2 * WST;
  static_assert(9 % TS == 0 && PLANE % 16 == 0 && SMEM <= 80 * 1024, "two workgroups per CU at least");
};

// this wave's outstanding loads (the weight DMA, the window pieces) and LDS stores are done; then everyone's are
__device__ __forceinline__ void halo_sync() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <int BN, int TS, int WMAX>
__global__ __launch_bounds__(256, 2) void conv3x3_f32_halo_kernel(const float* __restrict__ x,
                                                                  const u32v4* __restrict__ bs,
                                                                  const float* __restrict__ bias,
                                                                  const float* __restrict__ res,
                                                                  float* __restrict__ out, int B, int H, int W,
                                                                  int Cin, int Cout, int act, const pipe::Epi2 e2) {
  using C = HaloF32Cfg<BN, TS, WMAX>;
  __shared__ __attribute__((aligned(16))) char smem[C::SMEM];
  char* win = smem;
  char* wst = smem + C::WIN;
  const int HW = H * W;
  const long M = static_cast<long>(B) * HW;
  const int cin16 = Cin / kHaloCK, KT16 = 9 * cin16, NC = cin16;
  const int ntn = Cout / BN;
  const int wg = pipe::xcd_remap();
  const long m0 = static_cast<long>(wg / ntn) * kHaloBM;
  const int n0 = (wg % ntn) * BN;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, h = lane >> 5;
  const __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, static_cast<int>(M * Cin * 4), 0x00020000);
  const i32x4 br = pipe::rsrc(bs, static_cast<long>(Cout / 32) * KT16 * 3 * 1024);
  const long wb0 = m0 - (W + 1);                  // window row 0 <-> pixel wb0
  const int nrows = kHaloBM + 2 * W + 2;

  // per-tap byte offset (within a plane) of this lane's fragment: row pixel + (W + 1) + dy W + dx, channel half h;
  // the zero slot where the neighbour is outside the image (or the pixel past M)
  int a_off[9];
  {
    const long m = m0 + wid * 32 + l32;
    const int ok = conv_tap_mask(m, M, HW, H, W);
    const int r0 = wid * 32 + l32 + W + 1;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int r = r0 + (t / 3 - 1) * W + (t % 3 - 1);          // in [0, nrows) whenever the tap is in the image
      a_off[t] = ((ok >> t) & 1) ? r * 32 + ((h ^ ((r >> 3) & 1)) << 4) : C::NR * 32;
    }
  }

  // window pieces: piece = (row, channel quad q); source offset of chunk 0 or -1 (row outside the window / the
  // tensor: zeros through the buffer resource), LDS offset within plane 0
  int w_src[C::WP], w_dst[C::WP];
#pragma unroll
  for (int i = 0; i < C::WP; ++i) {
    const int piece = tid + 256 * i;
    const int row = piece >> 2, q = piece & 3;
    const long pix = wb0 + row;
    w_src[i] = (row < nrows && pix >= 0 && pix < M) ? static_cast<int>((pix * Cin + 4 * q) * 4) : -1;
    w_dst[i] = row < nrows ? row * 32 + (((q >> 1) ^ ((row >> 3) & 1)) << 4) + (q & 1) * 8 : -1;
  }
  uint4 rw[C::WP];
  auto load_win = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < C::WP; ++i) {
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(
          xr, w_src[i] >= 0 ? w_src[i] + chunk * (kHaloCK * 4) : pipe::kOOB, 0, 0);
      rw[i] = make_uint4(v[0], v[1], v[2], v[3]);
    }
  };
  auto store_win = [&]() {
#pragma unroll
    for (int i = 0; i < C::WP; ++i) {
      if (w_dst[i] < 0) continue;
      uint2 s0, s1, s2;
      split4(rw[i], s0, s1, s2);
      *reinterpret_cast<uint2*>(win + w_dst[i]) = s0;
      *reinterpret_cast<uint2*>(win + C::PLANE + w_dst[i]) = s1;
      *reinterpret_cast<uint2*>(win + 2 * C::PLANE + w_dst[i]) = s2;
    }
  };

  // weight pieces: stage piece q = wid + 4 c = (tap within the stage q / (3 FN), column block q / 3 % FN, plane q % 3)
  int b_off[C::W_PW];
#pragma unroll
  for (int c = 0; c < C::W_PW; ++c) {
    const int q = wid + 4 * c, tt = q / (3 * C::FN), j = q / 3 % C::FN, p = q % 3;
    b_off[c] = (((n0 / 32 + j) * KT16 + tt * cin16) * 3 + p) * 1024 + 16 * lane;
  }
  auto issue_w = [&](int chunk, int g) {             // stage (chunk, g): taps g TS .. g TS + TS - 1
    char* dst = wst + ((chunk + g) & 1) * C::WST;    // S is odd: the stage index chunk S + g has this parity
    const int kt0 = g * TS * cin16 + chunk;
#pragma unroll
    for (int c = 0; c < C::W_PW; ++c)
      if (C::QW % 4 == 0 || wid + 4 * c < C::QW)     // wave-uniform
        pipe::dma16(br, dst + (wid + 4 * c) * 1024, b_off[c] + kt0 * 3 * 1024);
  };

  f16v acc[1][C::FN];
#pragma unroll
  for (int j = 0; j < C::FN; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[0][j][e] = 0.f;

  if (tid < 3) *reinterpret_cast<uint4*>(win + tid * C::PLANE + C::NR * 32) = make_uint4(0, 0, 0, 0);
  load_win(0);
  issue_w(0, 0);
  store_win();
  for (int chunk = 0; chunk < NC; ++chunk) {
    const bool more = chunk + 1 < NC;
#pragma unroll
    for (int g = 0; g < C::S; ++g) {
      // the stage's weights and (g == 0) the chunk's window landed for everyone; everyone finished the previous
      // stage, whose weight buffer the next DMA refills
      halo_sync();
      if (g + 1 < C::S) issue_w(chunk, g + 1);
      else if (more) issue_w(chunk + 1, 0);
      if (g == 0 && more) load_win(chunk + 1);
      const char* wb = wst + ((chunk + g) & 1) * C::WST;
#pragma unroll
      for (int tt = 0; tt < TS; ++tt) {
        Split3 sa;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const uint4 u = *reinterpret_cast<const uint4*>(win + p * C::PLANE + a_off[g * TS + tt]);
          sa.p[p] = u32v4{u.x, u.y, u.z, u.w};
        }
#pragma unroll
        for (int j = 0; j < C::FN; ++j) {
          const char* bp = wb + (tt * C::FN + j) * 3 * 1024 + 16 * lane;
          Split3 sb;
#pragma unroll
          for (int p = 0; p < 3; ++p) {
            const uint4 u = *reinterpret_cast<const uint4*>(bp + p * 1024);
            sb.p[p] = u32v4{u.x, u.y, u.z, u.w};
          }
          acc[0][j] = mfma_x6(sb, sa, acc[0][j]);
        }
      }
      if (g == C::S - 1 && more) {
        // single-buffered window: every wave is done reading this chunk's planes before the next chunk's land
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        store_win();
      }
    }
  }
  pipe::store_tile<1, C::FN>(acc, out, bias, res, M, Cout, m0 + wid * 32, n0, act, e2);
}

template <int BN, int TS, int WMAX>
void launch_halo_f32(const float* x, const void* ws, const float* bias, const float* res, const pipe::Epi2& e2,
                     float* out, int B, int H, int W, int Cin, int Cout, int act, hipStream_t s) {
  const long M = static_cast<long>(B) * H * W;
  const long nwg = (M + kHaloBM - 1) / kHaloBM * (Cout / BN);
  hipLaunchKernelGGL((conv3x3_f32_halo_kernel<BN, TS, WMAX>), dim3(static_cast<unsigned>(nwg)), dim3(256), 0, s, x,
                     static_cast<const u32v4*>(ws), bias, res, out, B, H, W, Cin, Cout, act, e2);
}

template <int BN, int TS>
void launch_halo_f32_w(const float* x, const void* ws, const float* bias, const float* res, const pipe::Epi2& e2,
                       float* out, int B, int H, int W, int Cin, int Cout, int act, hipStream_t s) {
  if (W <= 20) launch_halo_f32<BN, TS, 20>(x, ws, bias, res, e2, out, B, H, W, Cin, Cout, act, s);
  else if (W <= 40) launch_halo_f32<BN, TS, 40>(x, ws, bias, res, e2, out, B, H, W, Cin, Cout, act, s);
  else launch_halo_f32<BN, TS, kHaloMaxW>(x, ws, bias, res, e2, out, B, H, W, Cin, Cout, act, s);
}

}  // namespace

bool conv3x3_f32_halo_supported(int H, int W, int Cin, int Cout) {
  return f32_mfma_mode() == 1 && H > 0 && W > 0 && W <= kHaloMaxW && Cin > 0 && Cin % kHaloCK == 0 &&
         (Cout == 32 || Cout == 64 || (Cout > 0 && Cout % 128 == 0));
}

void conv3x3_f32_halo(const float* x, const void* wsplit, const float* bias, const float* res, const float* res2,
                      long res2_rows, const float* mask, float* out, int B, int H, int W, int Cin, int Cout, int act,
                      hipStream_t s) {
  if (static_cast<long>(B) * H * W == 0) return;
  const pipe::Epi2 e2{res2, res2_rows, mask};
  // taps per weight stage, measured (docs/PERF_LOG.md): 64 outputs with one tap per stage (40 KB of LDS at W = 80:
  // four workgroups per CU) 470-490 us against 515-540 us with three (65 KB, two per CU) on the 76 x 80 32 -> 64
  // conv; 32 outputs the same either way (three: a third of the barriers); 128 outputs fit one tap only
  if (Cout == 32) launch_halo_f32_w<32, 3>(x, wsplit, bias, res, e2, out, B, H, W, Cin, Cout, act, s);
  else if (Cout == 64) launch_halo_f32_w<64, 1>(x, wsplit, bias, res, e2, out, B, H, W, Cin, Cout, act, s);
  else launch_halo_f32_w<128, 1>(x, wsplit, bias, res, e2, out, B, H, W, Cin, Cout, act, s);
}

}  // namespace as
