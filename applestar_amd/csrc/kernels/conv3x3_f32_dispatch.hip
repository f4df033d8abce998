// Which kernel runs an fp32 3 x 3 conv on pre-split weight planes (conv3x3_f32_psb): the switches, the support
// predicate and the choice, in one place.  Host code only; the kernels and their launchers are in
// conv3x3_f32_halo.hip, conv3x3_f32_v2.hip and gemm_f32_psb.hip.
//
// The decision, in order:
//   0. conv3x3_f32_psb_supported(M, Cin, Cout) is the caller's gate (native.py, the bindings): Cin % 16 (every
//      16-deep K-step inside one tap), 32-bit buffer offsets, and Cout % 128 - or Cout 64 / 32 while the ring
//      kernel is on (only it and the halo kernel have the narrow tiles).  Convs outside it run on the plain-weight
//      kernels of conv3x3_f32.hip (f32_mfma_mode 0-3, the narrow direct kernel).
//   1. halo window (conv3x3_f32_halo): where conv3x3_f32_halo_supported (split mode, W <= 80, Cout 32 / 64 /
//      128-multiples) and the output width's bit of conv_halo_f32_mode is set (APPLESTAR_CONV_HALO_F32 /
//      set_conv_halo_f32_mode; bits 1 = 32, 2 = 64, 4 = 128-multiples; default 7 - the measured choice,
//      docs/PERF_LOG.md; 0 = never).
//   2. LDS ring for both operands (conv3x3_f32_v2), variant conv_v2_variant() (APPLESTAR_CONV_V2, default 2:
//      4 x 1 waves, 2 stages, 4 workgroups per CU: 218 vs 235 us on the ResBlock conv, profiles/r8d_conv_v2.jsonl),
//      unless that switch is negative.
//   3. register-streamed weight planes (conv3x3_f32_psb_stream, gemm_f32_psb.hip): APPLESTAR_CONV_V2=-1.
#include <cstdlib>

#include "../kernels.h"

namespace as {
namespace {

int& halo_f32_ref() {
  static int v = [] {
    const char* e = std::getenv("APPLESTAR_CONV_HALO_F32");
    return e ? std::atoi(e) & 7 : 7;
  }();
  return v;
}

int conv_v2_variant() {
  static const int v = [] {
    const char* e = std::getenv("APPLESTAR_CONV_V2");
    return e ? std::atoi(e) : 2;
  }();
  return v;
}

}  // namespace

int conv_halo_f32_mode() { return halo_f32_ref(); }
void set_conv_halo_f32_mode(int mode) { halo_f32_ref() = mode & 7; }

bool conv3x3_f32_psb_supported(long M, int Cin, int Cout) {
  return (Cout % 128 == 0 || ((Cout == 64 || Cout == 32) && conv_v2_variant() >= 0)) && Cin % 16 == 0 && Cin > 0 &&
         M * Cin * 4 < 0x7ffffff0L && presplit_b_bytes(Cout, 9 * Cin) < 0x7ffffff0L && M * Cout < 0x7ffffff0L;
}

bool conv3x3_f32_halo_selected(int H, int W, int Cin, int Cout) {
  const int bit = Cout == 32 ? 1 : (Cout == 64 ? 2 : 4);
  return (conv_halo_f32_mode() & bit) != 0 && conv3x3_f32_halo_supported(H, W, Cin, Cout);
}

void conv3x3_f32_psb(const float* x, const void* wsplit, const float* bias, const float* res, const float* res2,
                     long res2_rows, const float* mask, float* out, int B, int H, int W, int Cin, int Cout, int act,
                     hipStream_t s) {
  if (conv3x3_f32_halo_selected(H, W, Cin, Cout))
    conv3x3_f32_halo(x, wsplit, bias, res, res2, res2_rows, mask, out, B, H, W, Cin, Cout, act, s);
  else if (conv_v2_variant() >= 0)
    conv3x3_f32_v2(x, wsplit, bias, res, res2, res2_rows, mask, out, B, H, W, Cin, Cout, act, conv_v2_variant(), s);
  else
    conv3x3_f32_psb_stream(x, wsplit, bias, res, res2, res2_rows, mask, out, B, H, W, Cin, Cout, act, s);
}

}  // namespace as
