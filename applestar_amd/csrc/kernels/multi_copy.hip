// Multi-tensor copy with dtype conversion: a few launches move every parameter gradient into its slot of
// a flat (bucket / fp32 master) buffer.  The gradient list of an RL step has ~470 tensors; copied one by
// one that is ~470 hipMemcpy / elementwise launches (rocprof r1_v13: 770 copyBuffer calls, 1.9 ms).
// Up to kCopyMaxT tensors travel BY VALUE in the kernel arguments (no host->device table upload, which
// would put a synchronising copy in the middle of the step); workgroup b finds its tensor by scanning
// the chunk prefix sums and copies one chunk of <= kCopyChunk elements.
#include "../common.h"
#include "../kernels.h"

namespace as {
namespace {

// element i of a converting copy's source: fp32, bf16, or an integer feature column (uint8 / int16, exact in fp32)
__device__ __forceinline__ float copy_src(const void* src, long i, unsigned char dts) {
  if (dts & 8) return static_cast<float>(static_cast<const unsigned char*>(src)[i]);
  if (dts & 16) return static_cast<float>(static_cast<const short*>(src)[i]);
  return (dts & 1) ? static_cast<const float*>(src)[i] : bf2f(static_cast<const bf16_t*>(src)[i]);
}

__global__ __launch_bounds__(256) void multi_copy_kernel(const CopyArgs a) {
  const int b = blockIdx.x;
  int t = 0;
  while (t + 1 < a.ntensors && a.chunk_start[t + 1] <= b) ++t;
  const void* src = a.src[t];
  void* dst = a.dst[t];
  if (a.dts[t] & 4) {
    // raw bytes (any dtype, n in bytes): 16-byte words when both ends and the length are 16-aligned
    const long i0 = static_cast<long>(b - a.chunk_start[t]) * kCopyRawChunk;
    const long i1 = i0 + kCopyRawChunk < a.n[t] ? i0 + kCopyRawChunk : a.n[t];
    const auto* s8 = static_cast<const unsigned char*>(src);
    auto* d8 = static_cast<unsigned char*>(dst);
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | a.n[t]) & 15) == 0) {
      // a full chunk: each thread's 16-B words all loaded before any is stored (one memory latency per chunk; the
      // dependent load -> store loop over 64-KB chunks moved the step's 126 MB of gradients at ~0.5 TB/s)
      constexpr int U = static_cast<int>(kCopyRawChunk / (16 * 256));
      if (i1 - i0 == kCopyRawChunk) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const uint4*>(s8 + i0 + 16 * (threadIdx.x + 256 * u));
#pragma unroll
        for (int u = 0; u < U; ++u) *reinterpret_cast<uint4*>(d8 + i0 + 16 * (threadIdx.x + 256 * u)) = v[u];
        return;
      }
      for (long i = i0 + 16 * threadIdx.x; i < i1; i += 16 * 256)
        *reinterpret_cast<uint4*>(d8 + i) = *reinterpret_cast<const uint4*>(s8 + i);
    } else {
      for (long i = i0 + threadIdx.x; i < i1; i += 256) d8[i] = s8[i];
    }
    return;
  }
  const long i0 = static_cast<long>(b - a.chunk_start[t]) * kCopyChunk;
  const long i1 = i0 + kCopyChunk < a.n[t] ? i0 + kCopyChunk : a.n[t];
  const bool df = (a.dts[t] & 2) != 0;
  const unsigned char dts = a.dts[t];
  if (i1 - i0 == kCopyChunk) {
    // a full chunk: the thread's 32 elements loaded before any is stored (see the raw path)
    constexpr int U = static_cast<int>(kCopyChunk / 256);
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = copy_src(src, i0 + threadIdx.x + 256 * u, dts);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + threadIdx.x + 256 * u;
      if (df) static_cast<float*>(dst)[i] = v[u];
      else static_cast<bf16_t*>(dst)[i] = f2bf(v[u]);
    }
    return;
  }
  for (long i = i0 + threadIdx.x; i < i1; i += 256) {
    const float v = copy_src(src, i, dts);
    if (df) static_cast<float*>(dst)[i] = v;
    else static_cast<bf16_t*>(dst)[i] = f2bf(v);
  }
}

// ---- gradient accumulation: dst = (dst + src) * scale, dst fp32, src fp32 or bf16 (widened exactly) -------------
// An add and a multiply, each rounded to fp32: the host replay (d + s.float()) * scale is bit-equal only while the
// two stay apart, so contraction into one fused multiply-add is switched off here (hipcc contracts by default).
__device__ __forceinline__ float acc_op(float d, float s, float scale) {
#pragma clang fp contract(off)
  const float t = d + s;
  return t * scale;
}

__device__ __forceinline__ float acc_src(const float* p, long i) { return p[i]; }
__device__ __forceinline__ float acc_src(const bf16_t* p, long i) { return bf2f(p[i]); }

// a 16-byte source word as its fp32 values: 4 floats, or 8 bf16 (element 2 k in the low half of 32-bit lane k)
__device__ __forceinline__ void acc_unpack(const uint4& w, float (&v)[4], const float*) {
  v[0] = __uint_as_float(w.x), v[1] = __uint_as_float(w.y), v[2] = __uint_as_float(w.z), v[3] = __uint_as_float(w.w);
}
__device__ __forceinline__ void acc_unpack(const uint4& w, float (&v)[8], const bf16_t*) {
  const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[2 * k] = __uint_as_float(u[k] << 16);
    v[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u);
  }
}

// one chunk [i0, i1) of one tensor; every element has one owner thread (no atomics: the launch is order-fixed)
template <typename S>
__device__ __forceinline__ void acc_chunk(float* dst, const S* src, long i0, long i1, float scale) {
  constexpr int V = 16 / static_cast<int>(sizeof(S));   // source elements per 16-byte word: 4 fp32, 8 bf16
  constexpr int Q = V / 4;                               // 16-byte words of dst per source word
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    // both ends 16-byte aligned (i0 is a multiple of kCopyChunk): 16-byte loads and stores
    if (i1 - i0 == kCopyChunk) {
      // a full chunk: every load of the thread's words issued before the first store (one memory latency per chunk)
      constexpr int U = static_cast<int>(kCopyChunk / (256 * V));
      uint4 sw[U];
      f32x4 dv[U][Q];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long i = i0 + static_cast<long>(V) * (threadIdx.x + 256 * u);
        sw[u] = *reinterpret_cast<const uint4*>(src + i);
#pragma unroll
        for (int q = 0; q < Q; ++q) dv[u][q] = *reinterpret_cast<const f32x4*>(dst + i + 4 * q);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long i = i0 + static_cast<long>(V) * (threadIdx.x + 256 * u);
        float sv[V];
        acc_unpack(sw[u], sv, src);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          f32x4 r;
#pragma unroll
          for (int k = 0; k < 4; ++k) r[k] = acc_op(dv[u][q][k], sv[4 * q + k], scale);
          *reinterpret_cast<f32x4*>(dst + i + 4 * q) = r;
        }
      }
      return;
    }
    // the tensor's last chunk: whole words, then the < V elements past them one by one
    const long nw = (i1 - i0) / V;
    for (long w = threadIdx.x; w < nw; w += 256) {
      const long i = i0 + w * V;
      const uint4 s4 = *reinterpret_cast<const uint4*>(src + i);
      f32x4 d4[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) d4[q] = *reinterpret_cast<const f32x4*>(dst + i + 4 * q);
      float sv[V];
      acc_unpack(s4, sv, src);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        f32x4 r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = acc_op(d4[q][k], sv[4 * q + k], scale);
        *reinterpret_cast<f32x4*>(dst + i + 4 * q) = r;
      }
    }
    for (long i = i0 + nw * V + threadIdx.x; i < i1; i += 256) dst[i] = acc_op(dst[i], acc_src(src, i), scale);
    return;
  }
  // an end off the 16-byte grid (a bucket view at an odd element offset): element by element
  if (i1 - i0 == kCopyChunk) {
    constexpr int U = static_cast<int>(kCopyChunk / 256);
    float sv[U], dv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + threadIdx.x + 256 * u;
      sv[u] = acc_src(src, i);
      dv[u] = dst[i];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) dst[i0 + threadIdx.x + 256 * u] = acc_op(dv[u], sv[u], scale);
    return;
  }
  for (long i = i0 + threadIdx.x; i < i1; i += 256) dst[i] = acc_op(dst[i], acc_src(src, i), scale);
}

// a slot without a source (a parameter that has no gradient in the window's closing micro-batch): dst *= scale, which
// is what (dst + nothing) * scale rounds to
__device__ __forceinline__ void scale_chunk(float* dst, long i0, long i1, float scale) {
  long i = i0 + threadIdx.x;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    const long nw = (i1 - i0) / 4;
    for (long w = threadIdx.x; w < nw; w += 256) {
      f32x4* p = reinterpret_cast<f32x4*>(dst + i0 + 4 * w);
      *p = *p * scale;
    }
    i += nw * 4;
  }
  for (; i < i1; i += 256) dst[i] *= scale;
}

__global__ __launch_bounds__(256) void multi_accumulate_kernel(const CopyArgs a, const float scale) {
  const int b = blockIdx.x;
  int t = 0;
  while (t + 1 < a.ntensors && a.chunk_start[t + 1] <= b) ++t;
  const long i0 = static_cast<long>(b - a.chunk_start[t]) * kCopyChunk;
  const long i1 = i0 + kCopyChunk < a.n[t] ? i0 + kCopyChunk : a.n[t];
  float* dst = static_cast<float*>(a.dst[t]);
  if (a.dts[t] & 32) scale_chunk(dst, i0, i1, scale);
  else if (a.dts[t] & 1) acc_chunk(dst, static_cast<const float*>(a.src[t]), i0, i1, scale);
  else acc_chunk(dst, static_cast<const bf16_t*>(a.src[t]), i0, i1, scale);
}


// ACC: dst (fp32) = (dst + the strided source element) * scale instead of the copy; every ACC branch is
// compile-time, so the copy's instantiation has the copy's inner loops and nothing else
template <bool ACC>
__device__ __forceinline__ void strided_body(const StridedCopyArgs& a, const float scale) {
  const int b = blockIdx.x;
  int t = 0;
  while (t + 1 < a.ntensors && a.chunk_start[t + 1] <= b) ++t;
  const int i0 = (b - a.chunk_start[t]) * static_cast<int>(kCopyChunk);
  const int i1 = i0 + static_cast<int>(kCopyChunk) < a.n[t] ? i0 + static_cast<int>(kCopyChunk) : a.n[t];
  const bool sf = (a.dts[t] & 1) != 0, df = (a.dts[t] & 2) != 0;
  if (a.dts[t] & 4) {
    // transpose form (dst [R, Cc] from src element (r, c) at base + r + c * S): a 64 x 128 tile through LDS,
    // read along r and written along c, both coalesced (the per-element path reads one row per lane)
    __shared__ float tile[128][65];
    const int R = a.size[t][2], Cc = a.size[t][3];
    const long S = a.stride[t][3];
    const int tiles_c = (Cc + 127) / 128, tb = b - a.chunk_start[t];
    const int r0 = (tb / tiles_c) * 64, c0 = (tb % tiles_c) * 128;
    for (int i = threadIdx.x; i < 128 * 64; i += 256) {
      const int cc = i >> 6, rr = i & 63, r = r0 + rr, c = c0 + cc;
      float v = 0.f;
      if (r < R && c < Cc) {
        const long off = a.base[t] + r + c * S;
        v = sf ? static_cast<const float*>(a.src[t])[off] : bf2f(static_cast<const bf16_t*>(a.src[t])[off]);
      }
      tile[cc][rr] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 128; i += 256) {
      const int rr = i >> 7, cc = i & 127, r = r0 + rr, c = c0 + cc;
      if (r < R && c < Cc) {
        const long o = static_cast<long>(r) * Cc + c;
        if constexpr (ACC) {
          float* d = static_cast<float*>(a.dst[t]);
          d[o] = acc_op(d[o], tile[cc][rr], scale);
        } else if (df) static_cast<float*>(a.dst[t])[o] = tile[cc][rr];
        else static_cast<bf16_t*>(a.dst[t])[o] = f2bf(tile[cc][rr]);
      }
    }
    return;
  }
  const int s1 = a.size[t][1], s2 = a.size[t][2], s3 = a.size[t][3];
  const long st0 = a.stride[t][0], st1 = a.stride[t][1], st2 = a.stride[t][2], st3 = a.stride[t][3];
  const void* src = a.src[t];
  void* dst = a.dst[t];
  constexpr int U = 8;   // loads of a pass issued before its stores
  for (int i = i0 + threadIdx.x; i < i1; i += 256 * U) {
    float v[U];
    [[maybe_unused]] float dv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = i + 256 * u;
      if (j < i1) {
        if constexpr (ACC) dv[u] = static_cast<const float*>(dst)[j];
        int r = j;
        const int c3 = r % s3;
        r /= s3;
        const int c2 = r % s2;
        r /= s2;
        const int c1 = r % s1;
        const int c0 = r / s1;
        const long off = a.base[t] + c0 * st0 + c1 * st1 + c2 * st2 + c3 * st3;
        v[u] = sf ? static_cast<const float*>(src)[off] : bf2f(static_cast<const bf16_t*>(src)[off]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = i + 256 * u;
      if (j < i1) {
        if constexpr (ACC) static_cast<float*>(dst)[j] = acc_op(dv[u], v[u], scale);
        else if (df) static_cast<float*>(dst)[j] = v[u];
        else static_cast<bf16_t*>(dst)[j] = f2bf(v[u]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void strided_copy_kernel(const StridedCopyArgs a) { strided_body<false>(a, 1.f); }

__global__ __launch_bounds__(256) void strided_accumulate_kernel(const StridedCopyArgs a, const float scale) {
  strided_body<true>(a, scale);
}

}  // namespace

void multi_copy(const CopyArgs& a, hipStream_t s) {
  const int nblk = a.chunk_start[a.ntensors];
  if (nblk > 0) hipLaunchKernelGGL(multi_copy_kernel, dim3(nblk), dim3(256), 0, s, a);
}

void multi_accumulate(const CopyArgs& a, float scale, hipStream_t s) {
  const int nblk = a.chunk_start[a.ntensors];
  if (nblk > 0) hipLaunchKernelGGL(multi_accumulate_kernel, dim3(nblk), dim3(256), 0, s, a, scale);
}

__global__ __launch_bounds__(256) void col_sum_kernel(const ColSumArgs a) {
  const int b = blockIdx.x;
  int p = 0;
  while (p + 1 < a.npieces && a.block_start[p + 1] <= b) ++p;
  const long n = a.rows * a.width[p];
  const int w = a.width[p], ns = a.nsrc[p];
  for (long i = static_cast<long>(b - a.block_start[p]) * 256 + threadIdx.x; i < n;
       i += static_cast<long>(a.block_start[p + 1] - a.block_start[p]) * 256) {
    const long r = i / w;
    const int c = static_cast<int>(i - r * w);
    float v = a.src[p][0][r * a.sld[p][0] + a.soff[p][0] + c];
    if (ns > 1) v += a.src[p][1][r * a.sld[p][1] + a.soff[p][1] + c];
    if (ns > 2) v += a.src[p][2][r * a.sld[p][2] + a.soff[p][2] + c];
    a.dst[p][r * a.dld[p] + a.doff[p] + c] = v;
  }
}

void col_sum(const ColSumArgs& a, hipStream_t s) {
  const int nblk = a.block_start[a.npieces];
  if (nblk > 0) hipLaunchKernelGGL(col_sum_kernel, dim3(nblk), dim3(256), 0, s, a);
}

void multi_strided_copy(const StridedCopyArgs& a, hipStream_t s) {
  const int nblk = a.chunk_start[a.ntensors];
  if (nblk > 0) hipLaunchKernelGGL(strided_copy_kernel, dim3(nblk), dim3(256), 0, s, a);
}

void multi_strided_accumulate(const StridedCopyArgs& a, float scale, hipStream_t s) {
  const int nblk = a.chunk_start[a.ntensors];
  if (nblk > 0) hipLaunchKernelGGL(strided_accumulate_kernel, dim3(nblk), dim3(256), 0, s, a, scale);
}

}  // namespace as
