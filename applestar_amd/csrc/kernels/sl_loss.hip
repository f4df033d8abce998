// Fused supervised (behaviour-cloning) loss, sl/loss.py: per-row cross entropy of the six action heads with its
// one-pass backward, and the loss tail (masked means, metrics, total, closed-form row gradients) in one workgroup.
//
// sl_ce_fwd: for every row r of logits l [R, C] (fp32 or bf16 storage) with label a[r] and smoothing eps, on the
// effective logits x (below):
//
//   m = max_i x_i, argmax = lowest index attaining m, lse = m + log sum_i exp(x_i - m)
//   nll = lse - x_a;   eps > 0: loss = (1 - eps) nll + eps (lse - mean_i x_i);   eps == 0: loss = nll
//
// All sums are taken on max-shifted values, so a row that is entirely -1e9 gives log C.  Labels outside [0, C) are
// clamped.  Outputs loss [R], argmax [R] (int64), stats [R, 2] = (m, log s).
// Rows that are switched off (row_on[r] == 0, or a padded / masked selected-units step) are never read: loss 0,
// argmax -1, stats 0.
// Selected-units form (R = b S, labels [b, S], len [b], on [b]): row (bi, si) is off when si >= len[bi] or
// on[bi] == 0.  With su_mask, x_i = -1e9 for every i in {labels[bi, j] : j < len[bi] - 1} except this row's own
// label (labels[bi, si] when si < len[bi] - 1): the forbidden set is a C-bit mask per row in LDS, built from the
// <= 64 labels of bi.  C <= 1024, S <= 64.
//
// sl_ce_bwd: dl_i = g_r (p_i - (1 - eps) [i == a] - eps / C), p_i = exp(x_i - m - log s); 0 at forbidden columns;
// rows with g_r == 0 or switched off write zeros without reading their logits.
//
// Rows of C <= 4096 use one wave each (4 rows per 256-thread workgroup); longer rows a whole workgroup.
//
// sl_loss_tail: one workgroup of 512 threads, every sum in a fixed order (per-thread strided partial, wave butterfly,
// the eight wave partials in index order; all in double), so the same input gives the same bits.  b <= 2048.  Layout of the info vector:
// the six head losses in HEADS order, selected_units_loss_norm, selected_units_end_flag_loss, action_type_acc,
// delay_distance_L1, queued_acc, selected_units_iou, target_unit_acc, target_location_distance_L2, total_loss.
#include <math.h>

#include "../common.h"
#include "../kernels.h"
#include "../row_reduce.h"

namespace as {
namespace {

constexpr int kForbWords = 32;      // selected-units form: C <= 1024 columns
constexpr int kNoIndex = 0x7fffffff;

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, kWave));
  return v;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

__device__ __forceinline__ double wave_sum_double(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

template <int TPR>
__device__ __forceinline__ int group_min_int(int v, int* red) {
  v = wave_min_int(v);
  if constexpr (TPR == 64) {
    return v;
  } else {
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return min(min(red[0], red[1]), min(red[2], red[3]));
  }
}

template <int TPR>
__device__ __forceinline__ double group_sum_double(double v, double* red) {
  v = wave_sum_double(v);
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

// Which rows are live, and for the selected-units form the forbidden-column mask of this wave's row.  Called by
// every thread of the workgroup (it synchronises).  Returns whether the row is read; `masked`: the mask applies.
template <bool SU>
__device__ __forceinline__ bool row_setup(const long* __restrict__ lab, const uint8_t* __restrict__ row_on,
                                          const long* __restrict__ su_len, const uint8_t* __restrict__ su_on, int S,
                                          int su_mask, long row, bool ok, int sub, int lt, int C,
                                          unsigned (*forb)[kForbWords], bool& masked) {
  masked = false;
  if constexpr (!SU) {
    return ok && (row_on == nullptr || row_on[row] != 0);
  } else {
    const long bi = ok ? row / S : 0;
    const int si = ok ? static_cast<int>(row % S) : 0;
    const long len = ok ? su_len[bi] : 0;
    const bool on = ok && si < len && su_on[bi] != 0;
    masked = on && su_mask != 0;
    if (lt < kForbWords) forb[sub][lt] = 0u;
    __syncthreads();
    if (masked && lt < S && lt < len - 1) {
      const long v = lab[bi * S + lt];
      if (v >= 0 && v < C) atomicOr(&forb[sub][v >> 5], 1u << (v & 31));
    }
    __syncthreads();
    if (masked && lt == 0 && si < len - 1) {
      const long v = lab[row];
      if (v >= 0 && v < C) forb[sub][v >> 5] &= ~(1u << (v & 31));
    }
    __syncthreads();
    return on;
  }
}

template <typename LT, int TPR, bool SU>
__global__ __launch_bounds__(256) void sl_ce_fwd_kernel(const LT* __restrict__ l, const long* __restrict__ lab,
                                                        const uint8_t* __restrict__ row_on,
                                                        const long* __restrict__ su_len,
                                                        const uint8_t* __restrict__ su_on, int S, int su_mask,
                                                        float eps, float* __restrict__ loss, long* __restrict__ amax,
                                                        float* __restrict__ stats, long R, int C) {
  constexpr int RPB = 256 / TPR;
  __shared__ float red[4];
  __shared__ int redi[4];
  __shared__ double redd[4];
  __shared__ unsigned forb[SU ? RPB : 1][kForbWords];
  const int sub = threadIdx.x / TPR, lt = threadIdx.x % TPR;
  const long row = static_cast<long>(blockIdx.x) * RPB + sub;
  const bool ok = row < R;
  bool masked;
  const bool on = row_setup<SU>(lab, row_on, su_len, su_on, S, su_mask, row, ok, sub, lt, C, forb, masked);
  if (!on) {   // a whole wave (TPR 64) or the whole workgroup (TPR 256) leaves together
    if (ok && lt == 0) {
      loss[row] = 0.f;
      amax[row] = -1;
      stats[2 * row] = 0.f;
      stats[2 * row + 1] = 0.f;
    }
    return;
  }
  const long base = row * static_cast<long>(C);
  auto X = [&](int i) -> float {
    float x = Cvt<LT>::load(l, base + i);
    if constexpr (SU) {
      if (masked && ((forb[sub][i >> 5] >> (i & 31)) & 1u)) x = -1e9f;
    }
    return x;
  };
  float best = -INFINITY;
  int idx = kNoIndex;
  for (int i = lt; i < C; i += TPR) {
    const float x = X(i);
    if (x > best) { best = x; idx = i; }   // ascending i: the lane keeps its lowest index
  }
  const float m = group_max<TPR>(best, red);
  int am = group_min_int<TPR>(best == m ? idx : kNoIndex, redi);
  if (am == kNoIndex) am = 0;
  float s = 0.f;
  double sx = 0.0;
  const bool smooth = eps > 0.f;
  for (int i = lt; i < C; i += TPR) {
    const float x = X(i) - m;
    s += expf(x);
    if (smooth) sx += static_cast<double>(x);
  }
  s = group_sum<TPR>(s, red);
  if (smooth) sx = group_sum_double<TPR>(sx, redd);
  if (lt == 0) {
    // one row's epilogue in double: the result is rounded to fp32 once
    const double logs = log(static_cast<double>(s));
    long a = lab[row];
    a = a < 0 ? 0 : (a >= C ? C - 1 : a);
    double v = logs - static_cast<double>(X(static_cast<int>(a)) - m);
    if (smooth) {
      const double e = static_cast<double>(eps);
      v = (1.0 - e) * v + e * (logs - sx / static_cast<double>(C));
    }
    loss[row] = static_cast<float>(v);
    amax[row] = am;
    stats[2 * row] = m;
    stats[2 * row + 1] = static_cast<float>(logs);
  }
}

template <typename LT, int TPR, bool SU>
__global__ __launch_bounds__(256) void sl_ce_bwd_kernel(const LT* __restrict__ l, const long* __restrict__ lab,
                                                        const uint8_t* __restrict__ row_on,
                                                        const long* __restrict__ su_len,
                                                        const uint8_t* __restrict__ su_on, int S, int su_mask,
                                                        float eps, const float* __restrict__ stats,
                                                        const float* __restrict__ g, LT* __restrict__ dl, long R,
                                                        int C) {
  constexpr int RPB = 256 / TPR;
  __shared__ unsigned forb[SU ? RPB : 1][kForbWords];
  const int sub = threadIdx.x / TPR, lt = threadIdx.x % TPR;
  const long row = static_cast<long>(blockIdx.x) * RPB + sub;
  const bool ok = row < R;
  bool masked;
  const bool on = row_setup<SU>(lab, row_on, su_len, su_on, S, su_mask, row, ok, sub, lt, C, forb, masked);
  if (!ok) return;
  const long base = row * static_cast<long>(C);
  const float gr = on ? g[row] : 0.f;
  if (gr == 0.f) {
    for (int i = lt; i < C; i += TPR) Cvt<LT>::store(dl, base + i, 0.f);
    return;
  }
  const float m = stats[2 * row], logs = stats[2 * row + 1];
  long a = lab[row];
  a = a < 0 ? 0 : (a >= C ? C - 1 : a);
  const float hit = 1.f - eps, flat = eps / static_cast<float>(C);
  for (int i = lt; i < C; i += TPR) {
    float d = 0.f;
    bool forbidden = false;
    if constexpr (SU) forbidden = masked && ((forb[sub][i >> 5] >> (i & 31)) & 1u);
    if (!forbidden) {
      const float p = __expf((Cvt<LT>::load(l, base + i) - m) - logs);
      d = gr * (p - (i == a ? hit : 0.f) - flat);
    }
    Cvt<LT>::store(dl, base + i, d);
  }
}

template <typename LT>
void ce_fwd_dispatch(const void* l, const long* lab, const uint8_t* row_on, const long* su_len, const uint8_t* su_on,
                     int S, int su_mask, float eps, float* loss, long* amax, float* stats, long R, int C,
                     hipStream_t s) {
  if (R == 0) return;
  const LT* lp = static_cast<const LT*>(l);
  if (su_len != nullptr) {
    hipLaunchKernelGGL((sl_ce_fwd_kernel<LT, 64, true>), dim3(static_cast<unsigned>((R + 3) / 4)), dim3(256), 0, s, lp,
                       lab, row_on, su_len, su_on, S, su_mask, eps, loss, amax, stats, R, C);
  } else if (C <= 4096) {
    hipLaunchKernelGGL((sl_ce_fwd_kernel<LT, 64, false>), dim3(static_cast<unsigned>((R + 3) / 4)), dim3(256), 0, s, lp,
                       lab, row_on, su_len, su_on, S, su_mask, eps, loss, amax, stats, R, C);
  } else {
    hipLaunchKernelGGL((sl_ce_fwd_kernel<LT, 256, false>), dim3(static_cast<unsigned>(R)), dim3(256), 0, s, lp, lab,
                       row_on, su_len, su_on, S, su_mask, eps, loss, amax, stats, R, C);
  }
}

template <typename LT>
void ce_bwd_dispatch(const void* l, const long* lab, const uint8_t* row_on, const long* su_len, const uint8_t* su_on,
                     int S, int su_mask, float eps, const float* stats, const float* g, void* dl, long R, int C,
                     hipStream_t s) {
  if (R == 0) return;
  const LT* lp = static_cast<const LT*>(l);
  LT* dp = static_cast<LT*>(dl);
  if (su_len != nullptr) {
    hipLaunchKernelGGL((sl_ce_bwd_kernel<LT, 64, true>), dim3(static_cast<unsigned>((R + 3) / 4)), dim3(256), 0, s, lp,
                       lab, row_on, su_len, su_on, S, su_mask, eps, stats, g, dp, R, C);
  } else if (C <= 4096) {
    hipLaunchKernelGGL((sl_ce_bwd_kernel<LT, 64, false>), dim3(static_cast<unsigned>((R + 3) / 4)), dim3(256), 0, s, lp,
                       lab, row_on, su_len, su_on, S, su_mask, eps, stats, g, dp, R, C);
  } else {
    hipLaunchKernelGGL((sl_ce_bwd_kernel<LT, 256, false>), dim3(static_cast<unsigned>(R)), dim3(256), 0, s, lp, lab,
                       row_on, su_len, su_on, S, su_mask, eps, stats, g, dp, R, C);
  }
}

// ------------------------------------------------------------------------------------------------ tail
constexpr int kTailT = 512;        // 1024 threads would cap the kernel at 128 VGPRs and spill
constexpr int kTailW = kTailT / kWave;
constexpr int kTailMaxB = 2048;

// every thread of the workgroup calls this; the result is the same in all of them (wave butterfly, then the wave
// partials in index order)
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum_double(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < kTailW; ++i) t += red[i];
  return t;
}

__global__ __launch_bounds__(kTailT) void sl_loss_tail_kernel(SLTailHeads A, const float* __restrict__ su_loss,
                                                              const long* __restrict__ su_lab,
                                                              const long* __restrict__ su_len,
                                                              const uint8_t* __restrict__ su_on,
                                                              const long* __restrict__ preds,
                                                              const long* __restrict__ ent_num,
                                                              const float* __restrict__ w,
                                                              const float* __restrict__ cr_scale, int b, int S, int n,
                                                              float* __restrict__ info, float* __restrict__ g_flat,
                                                              float* __restrict__ g_su) {
  __shared__ double red[kTailW];
  __shared__ unsigned s_p[kTailW][kForbWords], s_l[kTailW][kForbWords];
  __shared__ int s_live[kTailMaxB];      // live steps of each observation: min(len, S), 0 when masked out
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const double cr = static_cast<double>(cr_scale[0]);
  const bool cross = cr > 0.0;
  // info slots of the five flat heads (HEADS order skips selected_units at 3) and of their metrics
  constexpr int loss_slot[5] = {0, 1, 2, 4, 5};
  constexpr int metric_slot[5] = {8, 9, 10, 12, 13};

  // ---- the five flat heads in one pass over the rows (every load unconditional, so they overlap)
  double lm[5], sm[5], met[5];
#pragma unroll
  for (int f = 0; f < 5; ++f) { lm[f] = 0.0; sm[f] = 0.0; met[f] = 0.0; }
  double len_sum = 0.0, ef = 0.0, msum = 0.0;
  for (int r = tid; r < b; r += kTailT) {
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const bool on = A.mask[f][r] != 0;
      const float l = A.loss[f][r];
      const long p = A.amax[f][r], a = A.lab[f][r];
      lm[f] += on ? static_cast<double>(l) : 0.0;
      sm[f] += on ? 1.0 : 0.0;
      double m;
      if (f == 0 || f == 3) {
        m = p == a ? 1.0 : 0.0;
      } else if (f == 4) {
        const long dx = p % 160 - a % 160, dy = p / 160 - a / 160;
        m = static_cast<double>(sqrtf(static_cast<float>(dx * dx + dy * dy)));
      } else {
        m = static_cast<double>(p > a ? p - a : a - p);
      }
      met[f] += (f == 0 || on) ? m : 0.0;                 // the action-type accuracy ignores the mask
    }
    const long len = su_len[r];
    const bool on = su_on[r] != 0;
    long e = len - 1;
    e = e < 0 ? 0 : (e > S - 1 ? S - 1 : e);
    const float le = su_loss[static_cast<long>(r) * S + e];
    len_sum += static_cast<double>(len);
    ef += (on && e < len) ? static_cast<double>(le) : 0.0;
    msum += on ? 1.0 : 0.0;
    s_live[r] = on ? static_cast<int>(len < 0 ? 0 : (len > S ? S : len)) : 0;
  }
  double total = 0.0;
#pragma unroll
  for (int f = 0; f < 5; ++f) {
    const double lmf = block_sum(lm[f], red), smf = block_sum(sm[f], red), mf = block_sum(met[f], red);
    const double wh = static_cast<double>(w[loss_slot[f]]);
    const double scale = cross ? cr : 1.0 / fmax(smf, 1.0);
    const double lh = lmf * scale;
    total += wh * lh;
    const float gs = static_cast<float>(wh * scale);
    for (int r = tid; r < b; r += kTailT) g_flat[static_cast<long>(f) * b + r] = A.mask[f][r] != 0 ? gs : 0.f;
    if (tid == 0) {
      info[loss_slot[f]] = static_cast<float>(lh);
      info[metric_slot[f]] = static_cast<float>(f == 0 ? mf / static_cast<double>(b) : mf / (smf + 1e-6));
    }
  }
  len_sum = block_sum(len_sum, red);     // (its barriers also publish s_live)
  ef = block_sum(ef, red);
  msum = block_sum(msum, red);

  // ---- selected units: [b, S] row losses; a switched-off step counts as zero whatever it holds
  const int bs = b * S;                  // <= 2048 * 64
  const double w_su = static_cast<double>(w[3]);
  const double su_scale = cross ? cr : 1.0 / static_cast<double>(b);
  const float g_on = static_cast<float>(w_su * su_scale);
  double sum_all = 0.0;
#pragma unroll 4
  for (int i = tid; i < bs; i += kTailT) {
    const bool on = i % S < s_live[i / S];
    const float l = su_loss[i];
    sum_all += on ? static_cast<double>(l) : 0.0;
    g_su[i] = on ? g_on : 0.f;
  }
  sum_all = block_sum(sum_all, red);

  // ---- IoU of the predicted and the labelled unit sets, one wave per row (0 = "no unit"; sets hold value + 1)
  double iou = 0.0;
  if (preds != nullptr) {
    for (int r0 = 0; r0 < b; r0 += kTailW) {
      const int r = r0 + wv;
      const bool valid = r < b;
      long p = -1, pv = 0, lv = 0;       // set members as value + 1 in [1, n], 0 = none
      bool is_end = false;
      if (valid && lane < S) {
        p = preds[static_cast<long>(r) * S + lane];
        lv = su_lab[static_cast<long>(r) * S + lane];
        is_end = p == ent_num[r];
      }
      const unsigned long long ends = __ballot(is_end);
      const int count = ends != 0ull ? __ffsll(static_cast<long long>(ends)) : S;   // first end flag included
      if (valid && lane < S) {
        pv = lane < count ? p + 1 : 0;
        lv = lane < su_len[r] ? lv + 1 : 0;
        pv = pv < 1 ? 0 : (pv > n ? n : pv);
        lv = lv < 1 ? 0 : (lv > n ? n : lv);
      } else {
        lv = 0;
      }
      // the two sets as n-bit masks in LDS (bit v - 1 for member v): duplicates fall on one bit
      __syncthreads();
      if (lane < kForbWords) { s_p[wv][lane] = 0u; s_l[wv][lane] = 0u; }
      __syncthreads();
      if (pv != 0) atomicOr(&s_p[wv][(pv - 1) >> 5], 1u << ((pv - 1) & 31));
      if (lv != 0) atomicOr(&s_l[wv][(lv - 1) >> 5], 1u << ((lv - 1) & 31));
      __syncthreads();
      int ni = 0, nu = 0;
      if (lane < kForbWords) {
        const unsigned a = s_p[wv][lane], c = s_l[wv][lane];
        ni = __popc(a & c);
        nu = __popc(a | c);
      }
      ni = wave_sum_int(ni);
      nu = wave_sum_int(nu);
      if (valid && lane == 0 && su_on[r] != 0) iou += static_cast<double>(ni) / (static_cast<double>(nu) + 1e-6);
    }
  }
  iou = block_sum(iou, red);

  if (tid == 0) {
    const double lsu = sum_all * su_scale;
    total += w_su * lsu;
    info[3] = static_cast<float>(lsu);
    info[6] = static_cast<float>(sum_all / (len_sum + 1e-6));
    info[7] = static_cast<float>(ef / static_cast<double>(b));
    info[11] = preds != nullptr ? static_cast<float>(iou / (msum + 1e-6)) : 0.f;
    info[14] = static_cast<float>(total);
  }
}

}  // namespace

void sl_ce_fwd(const void* l, int l_dt, const long* lab, const uint8_t* row_on, const long* su_len,
               const uint8_t* su_on, int S, int su_mask, float eps, float* loss, long* amax, float* stats, long R, int C,
               hipStream_t s) {
  if (l_dt == DT_BF16) ce_fwd_dispatch<bf16_t>(l, lab, row_on, su_len, su_on, S, su_mask, eps, loss, amax, stats, R, C, s);
  else ce_fwd_dispatch<float>(l, lab, row_on, su_len, su_on, S, su_mask, eps, loss, amax, stats, R, C, s);
}

void sl_ce_bwd(const void* l, int l_dt, const long* lab, const uint8_t* row_on, const long* su_len,
               const uint8_t* su_on, int S, int su_mask, float eps, const float* stats, const float* g, void* dl, long R,
               int C, hipStream_t s) {
  if (l_dt == DT_BF16) ce_bwd_dispatch<bf16_t>(l, lab, row_on, su_len, su_on, S, su_mask, eps, stats, g, dl, R, C, s);
  else ce_bwd_dispatch<float>(l, lab, row_on, su_len, su_on, S, su_mask, eps, stats, g, dl, R, C, s);
}

int sl_ce_su_max_c() { return kForbWords * 32; }

void sl_loss_tail(const SLTailHeads& heads, const float* su_loss, const long* su_lab, const long* su_len,
                  const uint8_t* su_on, const long* preds, const long* ent_num, const float* w, const float* cr_scale,
                  int b, int S, int n, float* info, float* g_flat, float* g_su, hipStream_t s) {
  hipLaunchKernelGGL(sl_loss_tail_kernel, dim3(1), dim3(kTailT), 0, s, heads, su_loss, su_lab, su_len, su_on, preds,
                     ent_num, w, cr_scale, b, S, n, info, g_flat, g_su);
}

}  // namespace as
