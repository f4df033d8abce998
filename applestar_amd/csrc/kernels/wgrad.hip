// Weight (and bias) gradients of the tall-skinny GEMMs and 3x3 convolutions on the MFMA matrix cores.
//
//   dW[n, k] = sum_r dY[r, n] * X(r, k)          db[n] = sum_r dY[r, n]
//
// R (rows = batch * pixels or batch * entities) is 10^4 .. 10^7 while N x K is at most a few hundred
// squared, so the library GEMM (which tiles only the N x K output) runs a handful of workgroups on a
// 256-CU part (rocprof r1_v10: 5-workgroup hipBLASLt launches of 0.5 ms each for the 1x1 convs' dW).
// Here the reduction axis R is split over S slices (grid = N-tiles x K-tiles x S, >= ~1000 workgroups),
// each slice writes an fp32 partial, and the partials are summed afterwards (deterministic).
//
// X(r, k) has two forms:
//   * dense:   X is [R, K] row-major (nn.Linear / 1x1 conv on NHWC pixels);
//   * conv3x3: X is an NHWC [B, H, W, Cin] image, k = tap * Cin + c and X(r, k) = x[pixel r shifted by the
//     tap's (dy, dx)] (zero outside the image) - the implicit-GEMM weight gradient of a pad-1 3x3 conv in
//     the [Cout, 3, 3, Cin] (channels_last) weight order.  Replaces MIOpen's wrw solvers.
//
// Both MFMA operands are reduction-major in memory (row r holds all n / all k), so the tiles are staged
// row-major in LDS exactly as loaded (16-B chunks) and read back with the gfx950 transposed LDS read
// ds_read_b64_tr_b16: a 16-lane group receives a 4-row x 16-column block column-major, i.e. 4 consecutive
// reduction elements of 16 output columns.  The reduction index of fragment element j of lane group g is
// r = 4g + j (j < 4) and 16 + 4g + (j - 4) (j >= 4) - a permutation of 0..31 applied to both operands -
// so the two groups of one 32-lane half read 8 consecutive rows; with a row pitch of 72 dwords (BN = 128)
// or 40 dwords (BN = 64) those 8 rows start on 8 distinct 8-bank groups (conflict-free).
//
// Loads go through buffer descriptors: rows past the slice end, columns past N/K and taps outside the
// image get an out-of-range offset and read as zeros (no branches around loads).  The bias gradient is
// accumulated from the A fragments by the waves that own K-column 0 of K-tile 0.
#include <cstdlib>

#include "../common.h"
#include "../kernels.h"

namespace as {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf8v;
typedef __attribute__((ext_vector_type(4))) float f4;
typedef __attribute__((ext_vector_type(4))) short s4;
typedef __attribute__((address_space(3))) s4 lds_s4;

template <int BN_, int BK_>
struct WgCfg {
  static constexpr int BN = BN_, BK = BK_, BR = 64, NT = 256;
  static constexpr int TN = BN / 2, TK = BK / 2;       // 2 x 2 waves
  static constexpr int FN = TN / 16, FK = TK / 16;
  // LDS row pitch, bf16 elements: 72 / 56 / 40 / 24 dwords for 128 / 96 / 64 / 32 columns - each makes the
  // 8 consecutive rows of a transposed read start on 8 distinct 8-bank groups
  static constexpr int PA = BN + 16, PB = BK + 16;
  static constexpr int CHA = BN / 8, CHB = BK / 8;    // 16-B chunks per row
  static constexpr int A_IT = BR * CHA / NT, B_IT = BR * CHB / NT;
  static constexpr int STAGE = BR * (PA + PB);        // bf16 elements
  static constexpr int SMEM = 2 * STAGE * 2;
  static_assert(A_IT * NT == BR * CHA && B_IT * NT == BR * CHB && NT % CHA == 0, "tile / thread mismatch");
};

__device__ __forceinline__ bf8v tr_frag(const bf16_t* tile, int pitch, int col0, int lane) {
  // lanes 16g + 4q + p: rows 4g + q (first half) and 16 + 4g + q (second half), columns col0 + 4p .. + 3
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const bf16_t* a0 = tile + (4 * g + q) * pitch + col0 + 4 * p;
  const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(a0));
  const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(a0 + 16 * pitch));
  typedef __attribute__((ext_vector_type(8))) short s8;
  const s8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  bf8v r;
  __builtin_memcpy(&r, &v, 16);
  return r;
}

// WG_ABL: timing-ablation bits for tools/native/wgrad_ablation.cpp only (1: no row-stage loads after the
// first, 2: no partial-tile stores); 0 in every library build
#ifndef WG_ABL
#define WG_ABL 0
#endif

template <int BN, int BK, bool CONV>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgBatch P, long part_stride, long R, int N, int K, int H,
                                                    int W, int Cin, long rows_per_split, int tiles_n, int tiles_k,
                                                    int out_bf16) {
  using C = WgCfg<BN, BK>;
  // blockIdx.y selects one of a batch of independent problems of the same shape (one per launch otherwise)
  const bf16_t* __restrict__ dy = static_cast<const bf16_t*>(P.dy[blockIdx.y]);
  const bf16_t* __restrict__ x = static_cast<const bf16_t*>(P.x[blockIdx.y]);
  float* __restrict__ dw_part = P.dw[blockIdx.y];
  float* __restrict__ db_part = P.db[blockIdx.y];
  __shared__ __attribute__((aligned(16))) bf16_t smem[C::SMEM / 2];

  // XCD-aware remap: consecutive logical ids (the N x K tiles of one row slice, which read the same dY / X
  // rows) land on one XCD's L2
  const int wg = xcd_remap();
  const int tk = wg % tiles_k;
  const int tn = (wg / tiles_k) % tiles_n;
  const int s = wg / (tiles_k * tiles_n);
  const int n0 = tn * BN, k0 = tk * BK;
  const long r_begin = static_cast<long>(s) * rows_per_split;
  const long r_end = r_begin + rows_per_split < R ? r_begin + rows_per_split : R;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wn = wid >> 1, wk = wid & 1;

  const long HW = static_cast<long>(H) * W;
  const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(dy), 0,
                                                                      static_cast<int>(R * N * 2), 0x00020000);
  const long xbytes = CONV ? R * Cin * 2 : R * K * 2;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(x), 0,
                                                                      static_cast<int>(xbytes), 0x00020000);

  // per-thread chunk columns, fixed across row stages.  A: CHA divides NT, so every A chunk of a thread has
  // the same column.  B: CHB = 12 (BK = 96) does not divide NT, so each of a thread's B chunks has its own
  // column (and, for the conv form, its own tap).
  const int a_ch = tid % C::CHA;
  const int a_col = n0 + 8 * a_ch;
  const bool a_col_ok = a_col < N;
  int b_ch[C::B_IT], b_rr[C::B_IT], b_col[C::B_IT], b_c[C::B_IT], b_shift[C::B_IT], b_dy[C::B_IT], b_dx[C::B_IT];
#pragma unroll
  for (int i = 0; i < C::B_IT; ++i) {
    const int idx = tid + i * C::NT;
    b_ch[i] = idx % C::CHB;
    b_rr[i] = idx / C::CHB;
    b_col[i] = k0 + 8 * b_ch[i];
    b_c[i] = b_col[i];
    b_shift[i] = b_dy[i] = b_dx[i] = 0;
    if (CONV) {
      const int tap = b_col[i] / Cin;
      b_c[i] = b_col[i] - tap * Cin;
      b_dy[i] = tap / 3 - 1;
      b_dx[i] = tap % 3 - 1;
      b_shift[i] = b_dy[i] * W + b_dx[i];
    }
  }

  // conv form: image coordinates of each B chunk's row, advanced incrementally by BR rows per stage (a
  // 64-bit modulo + two divisions per chunk per stage were the bulk of the loop's VALU work)
  int cy[C::B_IT], cx[C::B_IT];
  const int adv_q = C::BR / W, adv_r = C::BR - (C::BR / W) * W;
  if (CONV) {
#pragma unroll
    for (int i = 0; i < C::B_IT; ++i) {
      const long r = r_begin + b_rr[i];
      const int rem = static_cast<int>(r % HW);
      cy[i] = rem / W;
      cx[i] = rem - cy[i] * W;
    }
  }
  uint4 ra[C::A_IT], rb[C::B_IT];
  auto load_regs = [&](long rs) {
#pragma unroll
    for (int i = 0; i < C::A_IT; ++i) {
      const long r = rs + (tid + i * C::NT) / C::CHA;
      const int off = (a_col_ok && r < r_end) ? static_cast<int>((r * N + a_col) * 2) : kOOB;
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(yr, off, 0, 0);
      ra[i] = make_uint4(v[0], v[1], v[2], v[3]);
    }
#pragma unroll
    for (int i = 0; i < C::B_IT; ++i) {
      const long r = rs + b_rr[i];
      const bool ok = b_col[i] < K && r < r_end;
      int off = kOOB;
      if (CONV) {
        const int yy = cy[i] + b_dy[i], xx = cx[i] + b_dx[i];
        if (ok && yy >= 0 && yy < H && xx >= 0 && xx < W)
          off = static_cast<int>(((r + b_shift[i]) * Cin + b_c[i]) * 2);
        // advance this chunk's row by BR for the next stage
        cx[i] += adv_r;
        cy[i] += adv_q;
        if (cx[i] >= W) {
          cx[i] -= W;
          cy[i] += 1;
        }
        while (cy[i] >= H) cy[i] -= H;
      } else if (ok) {
        off = static_cast<int>((r * K + b_col[i]) * 2);
      }
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0);
      rb[i] = make_uint4(v[0], v[1], v[2], v[3]);
    }
  };
  auto store_lds = [&](int st) {
    bf16_t* A = smem + st * C::STAGE;
    bf16_t* Bt = A + C::BR * C::PA;
#pragma unroll
    for (int i = 0; i < C::A_IT; ++i)
      *reinterpret_cast<uint4*>(A + ((tid + i * C::NT) / C::CHA) * C::PA + 8 * a_ch) = ra[i];
#pragma unroll
    for (int i = 0; i < C::B_IT; ++i)
      *reinterpret_cast<uint4*>(Bt + b_rr[i] * C::PB + 8 * b_ch[i]) = rb[i];
  };

  f4 acc[C::FN][C::FK];
#pragma unroll
  for (int i = 0; i < C::FN; ++i)
#pragma unroll
    for (int j = 0; j < C::FK; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = db_part != nullptr && tk == 0 && wk == 0;
  float bsum[C::FN];
#pragma unroll
  for (int i = 0; i < C::FN; ++i) bsum[i] = 0.f;

  const long nsteps = r_end > r_begin ? (r_end - r_begin + C::BR - 1) / C::BR : 0;
  if (nsteps > 0) {
    load_regs(r_begin);
    store_lds(0);
    __syncthreads();
  }
  for (long it = 0; it < nsteps; ++it) {
    const int cur = (WG_ABL & 1) ? 0 : static_cast<int>(it & 1);
    if (it + 1 < nsteps && !(WG_ABL & 1)) load_regs(r_begin + (it + 1) * C::BR);
    const bf16_t* A = smem + cur * C::STAGE;
    const bf16_t* Bt = A + C::BR * C::PA;
#pragma unroll
    for (int ks = 0; ks < C::BR / 32; ++ks) {
      bf8v af[C::FN], bfr[C::FK];
#pragma unroll
      for (int i = 0; i < C::FN; ++i) af[i] = tr_frag(A + ks * 32 * C::PA, C::PA, wn * C::TN + 16 * i, lane);
#pragma unroll
      for (int j = 0; j < C::FK; ++j) bfr[j] = tr_frag(Bt + ks * 32 * C::PB, C::PB, wk * C::TK + 16 * j, lane);
#pragma unroll
      for (int i = 0; i < C::FN; ++i)
#pragma unroll
        for (int j = 0; j < C::FK; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      if (do_bias) {
#pragma unroll
        for (int i = 0; i < C::FN; ++i)
#pragma unroll
          for (int e = 0; e < 8; ++e) bsum[i] += static_cast<float>(af[i][e]);
      }
    }
    if (it + 1 < nsteps && !(WG_ABL & 1)) store_lds(cur ^ 1);
    __syncthreads();
  }
  if (WG_ABL & 2) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < C::FN; ++i)
#pragma unroll
      for (int j = 0; j < C::FK; ++j) t += acc[i][j][0] + acc[i][j][3];
    if (t == 12345.f) dw_part[tid] = 1.f;
    return;
  }

  // epilogue: the fp32 tile goes through LDS (lane (g, i) of fragment (a, b) holds C[n = 16a + 4g + e][k = 16b + i])
  // and leaves as whole 16-B pieces of each row n, so a wave's stores cover full cache lines.  Scalar stores
  // straight from the fragments wrote 64-B pieces with 4x the store instructions: 24 of the 91 us of the
  // ResBlock conv dW (56 slices x 590 KB of partials, r2bx ablation).
  float* outp = dw_part + static_cast<long>(s) * part_stride;
  bf16_t* outb = reinterpret_cast<bf16_t*>(dw_part);
  const int lr = lane & 15, lg = lane >> 4;
  float* cs = reinterpret_cast<float*>(smem);
  constexpr int CP = C::BK + 4;                         // fp32 row pitch of the staged tile
  static_assert(C::BN * CP * 4 <= C::SMEM, "epilogue tile fits the staging LDS");
  __syncthreads();                                      // (the loop ends on a barrier; explicit for nsteps == 0)
#pragma unroll
  for (int i = 0; i < C::FN; ++i)
#pragma unroll
    for (int j = 0; j < C::FK; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        cs[(wn * C::TN + 16 * i + 4 * lg + e) * CP + wk * C::TK + 16 * j + lr] = acc[i][j][e];
  __syncthreads();
  constexpr int PR = C::BK / 4;                         // 4-float pieces per row
  for (int idx = tid; idx < C::BN * PR; idx += C::NT) {
    const int nn = idx / PR, kk = 4 * (idx % PR);
    const int n = n0 + nn, k = k0 + kk;
    if (n >= N || k >= K) continue;
    const float4 v = *reinterpret_cast<const float4*>(cs + nn * CP + kk);
    const long o = static_cast<long>(n) * K + k;
    if (k + 4 <= K && (K & 3) == 0) {
      if (out_bf16) {
        uint2 u;
        u.x = f2bf2(v.x, v.y);
        u.y = f2bf2(v.z, v.w);
        *reinterpret_cast<uint2*>(outb + o) = u;
      } else {
        *reinterpret_cast<float4*>(outp + o) = v;
      }
    } else {
      const float vv[4] = {v.x, v.y, v.z, v.w};
      for (int e = 0; e < 4 && k + e < K; ++e) {
        if (out_bf16) outb[o + e] = f2bf(vv[e]);
        else outp[o + e] = vv[e];
      }
    }
  }
  if (do_bias) {
#pragma unroll
    for (int i = 0; i < C::FN; ++i) {
      float v = bsum[i];
      v += __shfl_xor(v, 16, kWave);
      v += __shfl_xor(v, 32, kWave);
      const int n = n0 + wn * C::TN + 16 * i + lr;
      if (lg == 0 && n < N) {
        if (out_bf16) reinterpret_cast<bf16_t*>(db_part)[n] = f2bf(v);
        else db_part[static_cast<long>(s) * part_stride + n] = v;
      }
    }
  }
}

template <int BN, int BK, bool CONV>
void launch(const WgBatch& P, int nb, long ps, long R, int N, int K, int H, int W, int Cin, int S, long rps,
            int out_bf16, hipStream_t st) {
  const int tn = (N + BN - 1) / BN, tk = (K + BK - 1) / BK;
  const long nwg = static_cast<long>(tn) * tk * S;
  hipLaunchKernelGGL((wgrad_kernel<BN, BK, CONV>), dim3(static_cast<unsigned>(nwg), static_cast<unsigned>(nb)),
                     dim3(256), 0, st, P, ps, R, N, K, H, W, Cin, rps, tn, tk, out_bf16);
}

}  // namespace

namespace {
// tile choice: BN covers N with the least padding (32 / 64 / 128), BK in {64, 96, 128} minimises the padded
// K (3x3 convs: K = 9 Cin = 288 / 576 / 1152 -> BK 96 has no padding where 128 wastes up to 25 %)
int pick_bn(int N) { return N <= 32 ? 32 : (N <= 64 ? 64 : 128); }
int pick_bk(int K) {
  int best = 128;
  long best_pad = (K + 127) / 128 * 128L;
  for (int bk : {96, 64}) {
    const long pad = (K + bk - 1) / bk * static_cast<long>(bk);
    if (pad < best_pad) { best = bk; best_pad = pad; }
  }
  return best;
}
}  // namespace

// target workgroup count (APPLESTAR_WGRAD_WG, default 1024)
long wgrad_target_wg() {
  static const long v = [] {
    const char* e = std::getenv("APPLESTAR_WGRAD_WG");
    const long x = e ? std::atol(e) : 1024;
    return x >= 64 ? x : 1024;
  }();
  return v;
}

// few-row products (R < 2048): at least this many rows per slice (APPLESTAR_WGRAD_SMALL_R_BF16; 0 = one slice).
// Unlike the fp32 kernels (wgrad_f32.hip) the bf16 step did not move with 96 (26.95 / 27.10 vs 27.00 / 26.98 ms): off
long wgrad_small_r_rows() {
  static const long v = [] {
    const char* e = std::getenv("APPLESTAR_WGRAD_SMALL_R_BF16");
    return e ? std::atol(e) : 0L;
  }();
  return v;
}

int wgrad_splits(long R, int N, int K) {
  const int BN = pick_bn(N), BK = pick_bk(K);
  const long tiles = static_cast<long>((N + BN - 1) / BN) * ((K + BK - 1) / BK);
  const long target = wgrad_target_wg();
  long S = (target + tiles - 1) / tiles;               // ~target workgroups: 2 resident per CU
  // at least 256 rows (4 stages) per slice; short reductions (R < 2048, e.g. the 390-row policy / value
  // MLP gradients) take one slice so no partial-sum pass is launched at all
  const long small = wgrad_small_r_rows();
  const long max_s = R < 2048 ? (small > 0 && R >= 2 * small ? R / small : 1) : (R + 255) / 256;
  if (S > max_s) S = max_s;
  const long max_part = (8L << 20) / (static_cast<long>(N) * K);  // partials <= 32 MB (their sum is a pass)
  if (S > max_part) S = max_part;
  if (S < 1) S = 1;
  if (S > 4096) S = 4096;
  return static_cast<int>(S);
}

void wgrad_batched(const WgBatch& P, int nb, long part_stride, long R, int N, int K, int H, int W, int Cin, int S,
                   hipStream_t st, bool out_bf16) {
  const int ob = (out_bf16 && S == 1) ? 1 : 0;
  if (nb <= 0) return;
  long rps = (R + S - 1) / S;
  rps = (rps + 63) / 64 * 64;
  const bool conv = Cin > 0;
  const int bn = pick_bn(N), bk = pick_bk(K);
#define AS_WG(BNv, BKv)                                                                              \
  if (bn == BNv && bk == BKv) {                                                                      \
    if (conv) launch<BNv, BKv, true>(P, nb, part_stride, R, N, K, H, W, Cin, S, rps, ob, st);        \
    else launch<BNv, BKv, false>(P, nb, part_stride, R, N, K, H, W, Cin, S, rps, ob, st);            \
    return;                                                                                          \
  }
  AS_WG(128, 128) AS_WG(128, 96) AS_WG(128, 64)
  AS_WG(64, 128) AS_WG(64, 96) AS_WG(64, 64)
  AS_WG(32, 128) AS_WG(32, 96) AS_WG(32, 64)
#undef AS_WG
}

void wgrad(const void* dy, const void* x, float* dw_part, float* db_part, long part_stride, long R, int N, int K,
           int H, int W, int Cin, int S, hipStream_t st, bool out_bf16) {
  WgBatch P;
  P.dy[0] = dy;
  P.x[0] = x;
  P.dw[0] = dw_part;
  P.db[0] = db_part;
  wgrad_batched(P, 1, part_stride, R, N, K, H, W, Cin, S, st, out_bf16);
}

}  // namespace as
