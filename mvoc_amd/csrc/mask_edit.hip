// Matte edges at composition time: one pass of a separable grow / shrink / feather filter over [nplane][h][w] planes
// of fp16 (the latent masks) or uint8 (the image-size alphas).  A pass filters every plane along one axis with the window
// 2 * radius + 1; tap indices are clamped to the plane (replicated border), so a plane never reads its neighbour and no tap can
// leave the operand.  One work item per output element, a run-time tap loop, every load unconditional (the clamp is arithmetic:
// no load sits behind a data-dependent branch).  The rule is stated at mvoc_mask_filter_f16 in include/mvoc_hip.h:
//   max / min  the first tap, then every later tap that is strictly greater / smaller replaces it: exact in either type
//   mean fp16  acc = 0.0f; acc += (float)v for the taps in the order -radius .. radius; o = (half)(acc * inv), inv from the host:
//              one multiply that no add follows, so -ffp-contract=on has nothing to fuse; the product is rounded to fp32 first
//   mean u8    o = (2 * sum + n) / (2 * n), n = 2 * radius + 1, int32
// HBM- and latency-bound, a handful of launches per call: zero scratch and zero spills is the bar
// (tests/test_mask_edit_resources_cpu.py).  A translation unit of its own: the kernel census of the older units is pinned by tests.
//
// Bytes reported to the profiler (MvocProfScope, MVOC_FAM_MISC): 2 * n * sizeof(T) -- every element read once and written once,
// although an output reads 2 * radius + 1 of them (neighbouring outputs read neighbouring inputs, as the blend family counts).
#include "common.h"

namespace {

enum { OP_MAX = 0, OP_MIN = 1, OP_MEAN = 2 };

template <class T, int OP>
__global__ __launch_bounds__(256) void mask_filter_kernel(const T* __restrict__ src, T* __restrict__ dst, int h, int w, int radius,
                                                          int axis, float inv, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // (plane, y, x)
  if (i >= n) return;
  const int hw = h * w;
  const int pix = (int)(i % hw);
  const int y = pix / w, x = pix - y * w;
  const T* p = src + (i - pix);  // first element of the plane: 64-bit
  // along x: the row y, element x of w at stride 1; along y: the column x, element y of h at stride w
  const int pos = axis ? x : y, last = (axis ? w : h) - 1, stride = axis ? 1 : w, line = axis ? y * w : x;
  if (OP == OP_MEAN) {
    if (sizeof(T) == 2) {
      float acc = 0.0f;
      for (int d = -radius; d <= radius; ++d) acc += (float)p[line + min(max(pos + d, 0), last) * stride];
      // the rule rounds the product to fp32 and then to fp16.  Left alone, hipcc folds the multiply and the conversion into one
      // v_fma_mixlo_f16, which rounds the exact product once: another result where the fp32 product lands on an fp16 tie.  The
      // opaque copy keeps the two roundings apart.
      float prod = acc * inv;
      asm volatile("" : "+v"(prod));
      dst[i] = (T)prod;
    } else {
      int sum = 0;  // at most 129 * 255
      for (int d = -radius; d <= radius; ++d) sum += (int)p[line + min(max(pos + d, 0), last) * stride];
      const int cnt = 2 * radius + 1;
      dst[i] = (T)((2 * sum + cnt) / (2 * cnt));
    }
  } else {
    T o = p[line + max(pos - radius, 0) * stride];
    for (int d = 1 - radius; d <= radius; ++d) {
      const T v = p[line + min(max(pos + d, 0), last) * stride];
      o = (OP == OP_MAX ? v > o : v < o) ? v : o;  // a select, not a branch; ties (and -0 / +0) keep the earlier tap
    }
    dst[i] = o;
  }
}

template <class T>
int mask_filter(const char* name, const void* src, void* dst, int32_t nplane, int32_t h, int32_t w, int32_t op, int32_t radius,
                int32_t axis, float inv, void* stream) {
  MVOC_REQUIRE(src && dst, -1, "%s: null operand", name);
  MVOC_REQUIRE(src != dst, -1, "%s: in place (src == dst) is not supported", name);
  MVOC_REQUIRE(nplane > 0 && h > 0 && w > 0, -1, "%s: bad dims (nplane %d, h %d, w %d)", name, nplane, h, w);
  MVOC_REQUIRE(op >= 0 && op <= 2 && axis >= 0 && axis <= 1, -1, "%s: op %d not in [0, 2] or axis %d not in [0, 1]", name, op, axis);
  MVOC_REQUIRE(radius >= 0 && radius <= 64, -2, "%s: radius %d not in [0, 64]", name, radius);
  MVOC_REQUIRE((long)h * w < 0x80000000L, -2, "%s: h * w does not fit an int", name);
  const long n = (long)nplane * h * w;
  const long nblk = (n + 255) / 256;
  MVOC_REQUIRE(nblk < 0x7fffffffL, -2, "%s: grid too large", name);
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * n * sizeof(T));
  const dim3 grid((unsigned)nblk), block(256);
  const T* a = (const T*)src;
  T* b = (T*)dst;
  if (op == OP_MAX) hipLaunchKernelGGL((mask_filter_kernel<T, OP_MAX>), grid, block, 0, s, a, b, (int)h, (int)w, (int)radius, (int)axis, inv, n);
  else if (op == OP_MIN) hipLaunchKernelGGL((mask_filter_kernel<T, OP_MIN>), grid, block, 0, s, a, b, (int)h, (int)w, (int)radius, (int)axis, inv, n);
  else hipLaunchKernelGGL((mask_filter_kernel<T, OP_MEAN>), grid, block, 0, s, a, b, (int)h, (int)w, (int)radius, (int)axis, inv, n);
  return mvoc_check_launch("mask_filter_kernel");
}

}  // namespace

extern "C" int mvoc_mask_filter_f16(const void* src, void* dst, int32_t nplane, int32_t h, int32_t w, int32_t op, int32_t radius,
                                    int32_t axis, float inv, void* stream) {
  return mask_filter<half_t>("mask_filter_f16", src, dst, nplane, h, w, op, radius, axis, inv, stream);
}

extern "C" int mvoc_mask_filter_u8(const void* src, void* dst, int32_t nplane, int32_t h, int32_t w, int32_t op, int32_t radius,
                                   int32_t axis, void* stream) {
  return mask_filter<unsigned char>("mask_filter_u8", src, dst, nplane, h, w, op, radius, axis, 0.0f, stream);
}
