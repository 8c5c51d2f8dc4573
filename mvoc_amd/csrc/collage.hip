// The main conditioning frames of a composition, built from the sources under the call's own placement: the
// background frame with every object alpha-blended over it at the pixels a tap table names, 8-bit RGB, integers only.  The table
// is the TAPS form of DESIGN.md 6r at the IMAGE site (taps_src of pnp_blend.h decodes the same words for the fp16 planes); the
// nearest filter comes as degenerate taps (q = 0).  One work item per destination pixel, all three channels, a run-time object loop
// (later objects lie in front).  Per object the table entry is one int2 load and the sixteen byte loads of the four taps (three
// colours and the alpha each) are issued without a branch: a tap outside the plane reads the plane's pixel 0 and is ANDed to 0,
// so no table content can cause a read outside the planes.  A weight field above 256 counts as 256, so every sample is a byte
// and nothing leaves int32 (taps_src of the fp16 family does NOT clamp: the decodings agree for q <= 256 only).  HBM- and latency-bound, once per call: zero scratch and zero spills is the bar
// (tests/test_collage_resources_cpu.py).  A translation unit of its own, last in the link order: the kernel census of the older
// units is pinned by tests.
//
// Bytes reported to the profiler (MvocProfScope, MVOC_FAM_MISC): F * H * W * (3 + 3 + nobj * (8 + 3 + 1)) -- the background read,
// the frame written, and per object its table entry, its colours and its alpha, every object pixel counted once although a
// destination reads up to four of them (neighbouring destinations read neighbouring sources, as the blend family counts).
#include "common.h"

namespace {

// S(v) of the rule: the four tap values under the weights qx, qy in [0, 256] -> 0..255; at most 255 * 65536 + 32768 < 2^31
__device__ __forceinline__ unsigned sample8(unsigned v00, unsigned v01, unsigned v10, unsigned v11, unsigned qx, unsigned qy) {
  return ((v00 * (256u - qx) + v01 * qx) * (256u - qy) + (v10 * (256u - qx) + v11 * qx) * qy + 32768u) >> 16;
}

__global__ __launch_bounds__(256) void collage_rgb_u8_kernel(const unsigned char* __restrict__ bg, const unsigned char* __restrict__ objs,
                                                             const unsigned char* __restrict__ alpha, unsigned char* __restrict__ out,
                                                             int nobj, int frames, int h, int w, const int* __restrict__ taps, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // (f, y, x)
  if (i >= n) return;
  const int hw = h * w;
  const int pix = (int)(i % hw);
  const long f = i / hw;
  unsigned o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = bg[i * 3 + c];
  for (int j = 0; j < nobj; ++j) {
    const long plane = ((long)j * frames + f) * hw;  // first pixel of (object, frame): 64-bit
    const int2 t = *reinterpret_cast<const int2*>(taps + (plane + pix) * 2);
    const unsigned r0 = ((unsigned)t.x >> 16) - 1u, c0 = ((unsigned)t.x & 0xffffu) - 1u;
    const unsigned r1 = r0 + 1u, c1 = c0 + 1u;
    const bool ri0 = r0 < (unsigned)h, ri1 = r1 < (unsigned)h, ci0 = c0 < (unsigned)w, ci1 = c1 < (unsigned)w;
    const bool in[4] = {ri0 && ci0, ri0 && ci1, ri1 && ci0, ri1 && ci1};
    const unsigned at[4] = {r0 * w + c0, r0 * w + c1, r1 * w + c0, r1 * w + c1};
    const unsigned qy = min(((unsigned)t.y >> 16) & 0x1ffu, 256u), qx = min((unsigned)t.y & 0x1ffu, 256u);
    const unsigned char* ap = alpha + plane;
    const unsigned char* cp = objs + plane * 3;
    unsigned a[4], v[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned s = in[k] ? at[k] : 0u;   // outside: pixel 0 (always in bounds) ...
      const unsigned m = in[k] ? 0xffu : 0u;   // ... and the loaded byte is ANDed to 0
      a[k] = ap[s] & m;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[k][c] = cp[(long)s * 3 + c] & m;
    }
    const unsigned al = sample8(a[0], a[1], a[2], a[3], qx, qy);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      o[c] = (o[c] * (255u - al) + sample8(v[0][c], v[1][c], v[2][c], v[3][c], qx, qy) * al + 127u) / 255u;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[i * 3 + c] = (unsigned char)o[c];
}

}  // namespace

extern "C" int mvoc_collage_rgb_u8(const void* bg, const void* objs, const void* alpha, void* out, int32_t nobj, int32_t frames,
                                   int32_t h, int32_t w, const int32_t* taps, void* stream) {
  MVOC_REQUIRE(bg && objs && alpha && out && taps, -1, "collage: null operand");
  MVOC_REQUIRE(out != bg && out != objs && out != alpha && out != (const void*)taps, -1,
               "collage: out aliases an input (in place is not supported)");
  MVOC_REQUIRE(nobj >= 1 && nobj <= 16 && frames > 0 && h > 0 && w > 0, -1,
               "collage: nobj %d not in [1, 16] or bad dims (frames %d, h %d, w %d)", nobj, frames, h, w);
  MVOC_REQUIRE(h < 65535 && w < 65535, -2, "collage: h %d or w %d does not fit the 16-bit tap fields (< 65535)", h, w);
  MVOC_REQUIRE((long)h * w < 0x80000000L, -2, "collage: h * w does not fit an int");
  const long n = (long)frames * h * w;
  const long nblk = (n + 255) / 256;
  MVOC_REQUIRE(nblk < 0x7fffffffL, -2, "collage: grid too large");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, (double)n * (6.0 + 12.0 * nobj));
  hipLaunchKernelGGL(collage_rgb_u8_kernel, dim3((unsigned)nblk), dim3(256), 0, s, (const unsigned char*)bg, (const unsigned char*)objs,
                     (const unsigned char*)alpha, (unsigned char*)out, (int)nobj, (int)frames, (int)h, (int)w, (const int*)taps, n);
  return mvoc_check_launch("collage_rgb_u8_kernel");
}
