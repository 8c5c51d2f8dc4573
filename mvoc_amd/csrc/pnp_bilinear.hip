// Bilinear sampling of warped objects at composition time: the blend-scatter family with the TAPS object load.
// Object j of frame f is read at the four pixels a tap table names for every destination pixel and interpolated with fixed-point
// weights q / 256 on a chain of correctly rounded fp16 operations (lerp16_h, three times: top row, bottom row, between them), so
// the chunks hold the bits the unplaced entries write on sources that were interpolated beforehand by the same chain.  The
// kernels are blend_scatter<L, TAPS, true, NOBJ> composed from the pieces of pnp_blend.h exactly as pnp_warp.hip composes its
// MAP2 kernels.  A translation unit of its own: the kernel census of pnp.o, pnp_variants2.o and pnp_warp.o is pinned by tests.
// It holds the kernels and one call per entry: the form's row (BILINEAR) and the bodies of the entries and of the mover (run_entry,
// move_planes) are in pnp_blend.h, as for pnp.hip, pnp_variants2.hip and pnp_warp.hip.
//
// Bytes reported to the profiler (MvocProfScope): those of the _warped entries with the table term 8 * nobj * F * H * W -- every
// DISTINCT object chunk is counted once although a destination pixel reads up to four of its pixels (neighbouring destinations
// read neighbouring sources: the lines are shared through the caches, as the family counts repeated reads of one chunk).
#include "pnp_blend.h"

namespace {

template <int NOBJ>
__global__ __launch_bounds__(256) void pnp_tokens_bilinear_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                                  const int* __restrict__ taps) {
  blend_scatter<Tokens, TAPS, true, NOBJ>(p, nvar, active, taps);
}

template <int VEC, int NOBJ>
__global__ __launch_bounds__(256) void pnp_nchw_bilinear_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                                const int* __restrict__ taps) {
  blend_scatter<Nchw<VEC>, TAPS, true, NOBJ>(p, nvar, active, taps);
}

// zero-filled per-frame bilinear gather of [nplane][F][h][w] through a tap table: dst[pl, f, pix] = the chain of taps_value on
// the four taps of taps_f[pix] (a tap outside the plane is +0.0; nothing inside: 0); taps = F rows of h * w int32 pairs on the
// device, shared by the planes
__global__ __launch_bounds__(256) void gather_planes_bilinear_kernel(const half_t* __restrict__ src, half_t* __restrict__ dst,
                                                                     int frames, int h, int w, const int* __restrict__ taps, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int hw = h * w;
  const int pix = (int)(i % hw);
  const long pf = i / hw;  // pl * frames + f
  const int f = (int)(pf % frames);
  const int py = pix / w, px = pix - py * w;
  const Taps t = taps_src(taps, 0, frames, f, py, px, h, w);
  const half_t* pl = src + pf * hw;
  half_t v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = pl[t.s[k]];
  dst[i] = taps_value(t, v[0], v[1], v[2], v[3]);
}

}  // namespace

// run_entry / move_planes (pnp_blend.h) on the BILINEAR form: the _warped contract with the tap table in place of the 2-D map,
// and the form's limits on height * width and on the 16-bit tap fields
extern "C" int mvoc_pnp_blend_scatter_tokens_bilinear(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                      uint32_t active, const int32_t* taps, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_tokens_bilinear", "pnp_tokens_bilinear_kernel", BILINEAR, prepare_tokens, d, nsrc, obj_chunk,
                   nvar, active, taps, stream, [&](auto n, auto, const Launch& l, const PnpArgs& a) {
                     launch(pnp_tokens_bilinear_kernel<n.value>, l, a, (int)nvar, (unsigned)active, (const int*)taps);
                   });
}

extern "C" int mvoc_pnp_blend_scatter_nchw_bilinear(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                    uint32_t active, const int32_t* taps, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_nchw_bilinear", "pnp_nchw_bilinear_kernel", BILINEAR, prepare_nchw, d, nsrc, obj_chunk, nvar,
                   active, taps, stream, [&](auto n, auto v, const Launch& l, const PnpArgs& a) {
                     launch(pnp_nchw_bilinear_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active, (const int*)taps);
                   });
}

extern "C" int mvoc_gather_planes_bilinear_f16(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w,
                                               const int32_t* taps, void* stream) {
  return move_planes(BILINEAR, "gather_planes_bilinear_kernel", src, dst, nplane, frames, h, w, taps, stream,
                     [&](dim3 grid, hipStream_t s, long n) {
                       hipLaunchKernelGGL(gather_planes_bilinear_kernel, grid, dim3(256), 0, s, (const half_t*)src, (half_t*)dst,
                                          (int)frames, (int)h, (int)w, (const int*)taps, n);
                     });
}
