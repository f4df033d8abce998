// Order-fixed (bit-reproducible) forms of the scatter / gather-gradient sums, for gfx950.  Selected by
// ops.set_deterministic / APPLESTAR_DETERMINISTIC=1 only; the atomic kernels stay the default.  No kernel here uses
// a float atomic: every destination has one owner thread that adds its sources in an order fixed by the operands'
// shapes and index values, so a result depends on the operands alone (not on wave scheduling, on other work on the
// device or on what the allocator handed out).  Accumulation is fp32.
//
// table_grad_ordered: dT[v, :] = sum_u [idx[u] == v] src[u, :] for the small tables (pool_reduce.hip table_grad /
//   embed_relu_bwd).  A fixed grid: workgroup w owns the contiguous rows [w rpb, (w + 1) rpb).  Inside it the 256
//   threads are G = 256 / D row groups of D column threads; the V x D accumulator has K copies in LDS (as many as
//   64 KiB hold, at most G) and the G groups are split into K copies x J table-row classes: group (k, j) walks
//   the rows u = r0 + k, r0 + k + K, ... in ascending order and adds those with idx[u] % J == j into copy k, so no
//   two threads ever touch one LDS word.  The copies are then summed in copy order into the workgroup's partial
//   row, and column_reduce (fixed order) sums the partials.  One workgroup writes the result outright.
// gather_steps: out[b, s, :] = key[b, labels[b, s], :]; backward dkey[b, n, :] = sum of dout[b, s, :] over the steps
//   s with labels[b, s] == n in ascending s (one thread per (n, c); rows no label names are zero).  With B = 1 it is
//   the ordered gradient of a plain row gather table[idx] for tables too large for table_grad's LDS copies.
// scatter_connection: out[b, y, x, :] = sum of proj[b, u, :] over the units u at pixel (y, x) in ascending u,
//   starting from the first contribution; pixels with no unit are +0.  The first unit of a pixel owns it.
#include <algorithm>

#include "../common.h"
#include "../kernels.h"

namespace as {
namespace {

constexpr int kOrdLdsFloats = 16384;   // 64 KiB of accumulator copies
constexpr int kScMaxUnits = 2048;      // units per observation (pixel index staged in LDS)
constexpr int kScPixPerBlock = 8192;   // pixels per workgroup (occupancy bitmap in LDS)
constexpr int kGsChunk = 1024;         // labels of an observation staged in LDS per pass

// idt: 0 int64, 1 int32, 2 int16, 3 uint8, 4 int8 (bindings.cpp idx_dtype_code)
__device__ __forceinline__ long load_index(const void* p, int idt, long i) {
  switch (idt) {
    case 0: return static_cast<long>(static_cast<const int64_t*>(p)[i]);
    case 1: return static_cast<long>(static_cast<const int32_t*>(p)[i]);
    case 2: return static_cast<long>(static_cast<const int16_t*>(p)[i]);
    case 3: return static_cast<long>(static_cast<const uint8_t*>(p)[i]);
    default: return static_cast<long>(static_cast<const int8_t*>(p)[i]);
  }
}

__device__ __forceinline__ int clampi(long v, int hi) {   // to [0, hi]
  return static_cast<int>(v < 0 ? 0 : (v > hi ? hi : v));
}

// RELU = false: rows with idx outside [0, V) are skipped (table_grad).  RELU = true: idx is clamped to [0, V) and
// an element counts only where the forward output `out` is positive (embed_relu_bwd).
template <typename T, bool RELU>
__global__ __launch_bounds__(256) void table_grad_ordered_kernel(const T* __restrict__ src, const T* __restrict__ out,
                                                                 const void* __restrict__ idx, int idt,
                                                                 float* __restrict__ part, long U, int V, int D,
                                                                 long rpb, int Dc, int K, int J) {
  extern __shared__ float acc[];
  const int VD = V * D;
  for (int i = threadIdx.x; i < K * VD; i += 256) acc[i] = 0.f;
  __syncthreads();
  const int g = threadIdx.x / Dc, dl = threadIdx.x - g * Dc;
  if (g < K * J) {
    const int k = g % K, j = g / K;
    const long r0 = static_cast<long>(blockIdx.x) * rpb, r1 = min(r0 + rpb, U);
    float* a = acc + static_cast<long>(k) * VD;
    for (long u = r0 + k; u < r1; u += K) {
      long v = load_index(idx, idt, u);
      if (RELU) v = clampi(v, V - 1);
      else if (v < 0 || v >= V) continue;
      if (static_cast<int>(v % J) != j) continue;
      for (int d = dl; d < D; d += Dc) {
        const long e = u * D + d;
        if (RELU && !(Cvt<T>::load(out, e) > 0.f)) continue;
        a[static_cast<int>(v) * D + d] += Cvt<T>::load(src, e);
      }
    }
  }
  __syncthreads();
  float* dst = part + static_cast<long>(blockIdx.x) * VD;
  for (int i = threadIdx.x; i < VD; i += 256) {
    float s = acc[i];
    for (int k = 1; k < K; ++k) s += acc[k * VD + i];
    dst[i] = s;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void gather_steps_fwd_kernel(const T* __restrict__ key, const int64_t* __restrict__ labels,
                                                               T* __restrict__ out, long total, int N1, int S, int C) {
  for (long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<long>(gridDim.x) * 256) {
    const long bs = i / C;
    const int c = static_cast<int>(i - bs * C);
    const long b = bs / S;
    out[i] = key[(b * N1 + clampi(labels[bs], N1 - 1)) * C + c];
  }
}

// grid (ceil(N1 C / 256), B)
template <typename T>
__global__ __launch_bounds__(256) void gather_steps_bwd_kernel(const T* __restrict__ dout, const int64_t* __restrict__ labels,
                                                               T* __restrict__ dkey, int N1, int S, int C) {
  __shared__ int lab[kGsChunk];
  const long b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < N1 * C;
  const int n = live ? i / C : -1, c = live ? i - n * C : 0;
  const T* d = dout + b * S * C + c;
  float a = 0.f;
  for (int s0 = 0; s0 < S; s0 += kGsChunk) {
    const int ns = min(kGsChunk, S - s0);
    __syncthreads();
    for (int s = threadIdx.x; s < ns; s += 256) lab[s] = clampi(labels[b * S + s0 + s], N1 - 1);
    __syncthreads();
    for (int s = 0; s < ns; ++s)
      if (lab[s] == n) a += Cvt<T>::load(d, static_cast<long>(s0 + s) * C);
  }
  if (live) Cvt<T>::store(dkey, (b * N1 + n) * C + c, a);
}

// grid (B, ceil(HW / kScPixPerBlock)); workgroup (b, z) writes the pixels [z, z + 1) * kScPixPerBlock of observation b
template <typename T>
__global__ __launch_bounds__(256) void scatter_conn_fwd_kernel(const T* __restrict__ proj, const void* __restrict__ x,
                                                               int xdt, const void* __restrict__ y, int ydt,
                                                               T* __restrict__ out, int U, int C, int H, int W) {
  __shared__ int pix[kScMaxUnits];
  __shared__ unsigned char first[kScMaxUnits];
  __shared__ unsigned occ[kScPixPerBlock / 32];
  const long b = blockIdx.x;
  const int HW = H * W;
  const int p0 = blockIdx.y * kScPixPerBlock, p1 = min(p0 + kScPixPerBlock, HW);
  for (int i = threadIdx.x; i < kScPixPerBlock / 32; i += 256) occ[i] = 0u;
  for (int u = threadIdx.x; u < U; u += 256)
    pix[u] = clampi(load_index(y, ydt, b * U + u), H - 1) * W + clampi(load_index(x, xdt, b * U + u), W - 1);
  __syncthreads();
  for (int u = threadIdx.x; u < U; u += 256) {
    const int p = pix[u];
    bool f = p >= p0 && p < p1;
    if (f) {
      atomicOr(&occ[(p - p0) >> 5], 1u << ((p - p0) & 31));   // integer: order-free
      for (int u2 = 0; u2 < u; ++u2)
        if (pix[u2] == p) { f = false; break; }
    }
    first[u] = f ? 1 : 0;
  }
  __syncthreads();
  T* ob = out + b * HW * C;
  for (long i = threadIdx.x; i < static_cast<long>(p1 - p0) * C; i += 256) {
    const int p = static_cast<int>(i / C);
    if (!((occ[p >> 5] >> (p & 31)) & 1u)) Cvt<T>::store(ob, static_cast<long>(p0) * C + i, 0.f);
  }
  const T* pb = proj + b * U * C;
  for (int i = threadIdx.x; i < U * C; i += 256) {
    const int u = i / C, c = i - u * C;
    if (!first[u]) continue;
    const int p = pix[u];
    float a = Cvt<T>::load(pb, i);
    for (int u2 = u + 1; u2 < U; ++u2)
      if (pix[u2] == p) a += Cvt<T>::load(pb, static_cast<long>(u2) * C + c);
    Cvt<T>::store(ob, static_cast<long>(p) * C + c, a);
  }
}

// dproj[b, u, :] = dout[b, y, x, :] (dout NHWC)
template <typename T>
__global__ __launch_bounds__(256) void scatter_conn_bwd_kernel(const T* __restrict__ dout, const void* __restrict__ x,
                                                               int xdt, const void* __restrict__ y, int ydt,
                                                               T* __restrict__ dproj, long total, int U, int C, int H,
                                                               int W) {
  for (long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<long>(gridDim.x) * 256) {
    const long bu = i / C;
    const int c = static_cast<int>(i - bu * C);
    const long b = bu / U;
    const long p = static_cast<long>(clampi(load_index(y, ydt, bu), H - 1)) * W + clampi(load_index(x, xdt, bu), W - 1);
    dproj[i] = dout[(b * H * W + p) * C + c];
  }
}

unsigned flat_grid(long total) { return static_cast<unsigned>(std::min<long>((total + 255) / 256, 4096)); }

}  // namespace

int table_grad_ordered_blocks(long U, bool single) {
  if (single || U <= 0) return 1;
  const long rpb = std::max<long>((U + 255) / 256, 64);
  return static_cast<int>((U + rpb - 1) / rpb);
}

void table_grad_ordered(const void* src, const void* out_mask, int dt, const void* idx, int idt, float* part, long U,
                        int V, int D, int blocks, hipStream_t s) {
  const long rpb = blocks == 1 ? std::max<long>(U, 1) : std::max<long>((U + 255) / 256, 64);
  const int Dc = std::min(D, 256), G = 256 / Dc;
  const int K = std::max(1, std::min(G, kOrdLdsFloats / (V * D)));
  const int J = std::max(1, G / K);
  const size_t lds = static_cast<size_t>(K) * V * D * sizeof(float);
  const dim3 grid(static_cast<unsigned>(blocks));
#define AS_TG_LAUNCH(T, RELU)                                                                                       \
  hipLaunchKernelGGL((table_grad_ordered_kernel<T, RELU>), grid, dim3(256), lds, s, static_cast<const T*>(src),      \
                     static_cast<const T*>(out_mask), idx, idt, part, U, V, D, rpb, Dc, K, J)
  if (dt == DT_BF16) {
    if (out_mask) AS_TG_LAUNCH(bf16_t, true);
    else AS_TG_LAUNCH(bf16_t, false);
  } else {
    if (out_mask) AS_TG_LAUNCH(float, true);
    else AS_TG_LAUNCH(float, false);
  }
#undef AS_TG_LAUNCH
}

void gather_steps_fwd(const void* key, int dt, const int64_t* labels, void* out, long B, int N1, int S, int C,
                      hipStream_t s) {
  const long total = B * S * C;
  if (total == 0) return;
  if (dt == DT_BF16)
    hipLaunchKernelGGL(gather_steps_fwd_kernel<bf16_t>, dim3(flat_grid(total)), dim3(256), 0, s,
                       static_cast<const bf16_t*>(key), labels, static_cast<bf16_t*>(out), total, N1, S, C);
  else
    hipLaunchKernelGGL(gather_steps_fwd_kernel<float>, dim3(flat_grid(total)), dim3(256), 0, s,
                       static_cast<const float*>(key), labels, static_cast<float*>(out), total, N1, S, C);
}

void gather_steps_bwd(const void* dout, int dt, const int64_t* labels, void* dkey, long B, int N1, int S, int C,
                      hipStream_t s) {
  if (B == 0 || N1 * C == 0) return;
  const dim3 grid(static_cast<unsigned>((N1 * C + 255) / 256), static_cast<unsigned>(B));
  if (dt == DT_BF16)
    hipLaunchKernelGGL(gather_steps_bwd_kernel<bf16_t>, grid, dim3(256), 0, s, static_cast<const bf16_t*>(dout), labels,
                       static_cast<bf16_t*>(dkey), N1, S, C);
  else
    hipLaunchKernelGGL(gather_steps_bwd_kernel<float>, grid, dim3(256), 0, s, static_cast<const float*>(dout), labels,
                       static_cast<float*>(dkey), N1, S, C);
}

int scatter_conn_max_units() { return kScMaxUnits; }

void scatter_conn_fwd(const void* proj, int dt, const void* x, int xdt, const void* y, int ydt, void* out, long B, int U,
                      int C, int H, int W, hipStream_t s) {
  if (B == 0 || H * W * C == 0) return;
  const dim3 grid(static_cast<unsigned>(B), static_cast<unsigned>((H * W + kScPixPerBlock - 1) / kScPixPerBlock));
  if (dt == DT_BF16)
    hipLaunchKernelGGL(scatter_conn_fwd_kernel<bf16_t>, grid, dim3(256), 0, s, static_cast<const bf16_t*>(proj), x, xdt,
                       y, ydt, static_cast<bf16_t*>(out), U, C, H, W);
  else
    hipLaunchKernelGGL(scatter_conn_fwd_kernel<float>, grid, dim3(256), 0, s, static_cast<const float*>(proj), x, xdt, y,
                       ydt, static_cast<float*>(out), U, C, H, W);
}

void scatter_conn_bwd(const void* dout, int dt, const void* x, int xdt, const void* y, int ydt, void* dproj, long B,
                      int U, int C, int H, int W, hipStream_t s) {
  const long total = B * U * C;
  if (total == 0) return;
  if (dt == DT_BF16)
    hipLaunchKernelGGL(scatter_conn_bwd_kernel<bf16_t>, dim3(flat_grid(total)), dim3(256), 0, s,
                       static_cast<const bf16_t*>(dout), x, xdt, y, ydt, static_cast<bf16_t*>(dproj), total, U, C, H, W);
  else
    hipLaunchKernelGGL(scatter_conn_bwd_kernel<float>, dim3(flat_grid(total)), dim3(256), 0, s,
                       static_cast<const float*>(dout), x, xdt, y, ydt, static_cast<float*>(dproj), total, U, C, H, W);
}

}  // namespace as
