// Rotation of objects at composition time: the blend-scatter family with the MAP2 object load.  Object j of
// frame f is read at the source pixel a 2-D index map names for every destination pixel -- a rotation (or any affine map) is not
// separable into the per-axis maps of the _resampled entries.  The kernels are blend_scatter<L, MAP2, SEL, NOBJ> composed from the
// pieces of pnp_blend.h exactly as pnp.hip composes its _resampled kernels (<L, MAP, SEL, NOBJ>): one table load per pixel in
// place of two, the same gather, the same fp16 blend; only values move, so the chunks hold the bits the unplaced entries write on
// sources gathered beforehand.  A translation unit of its own: the kernel census of pnp.o is pinned by tests.  It holds the
// kernels and one call per entry: the form's row (WARPED) and the bodies of the entries and of the mover (run_entry, move_planes)
// are in pnp_blend.h, as for pnp.hip, pnp_variants2.hip and pnp_bilinear.hip.
#include "pnp_blend.h"

namespace {

template <int NOBJ>
__global__ __launch_bounds__(256) void pnp_tokens_warped_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                                const int* __restrict__ map) {
  blend_scatter<Tokens, MAP2, true, NOBJ>(p, nvar, active, map);
}

template <int VEC, int NOBJ>
__global__ __launch_bounds__(256) void pnp_nchw_warped_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                              const int* __restrict__ map) {
  blend_scatter<Nchw<VEC>, MAP2, true, NOBJ>(p, nvar, active, map);
}

// zero-filled per-frame gather of [nplane][F][h][w] through a 2-D map: dst[pl, f, pix] = src[pl, f, map_f[pix]] or 0 where the
// entry is outside the plane (compared unsigned: every int32 entry is safe); map = F rows of h * w int32 on the device, shared by
// the planes
__global__ __launch_bounds__(256) void gather_planes_warped_kernel(const half_t* __restrict__ src, half_t* __restrict__ dst,
                                                                   int frames, int hw, const int* __restrict__ map, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int pix = (int)(i % hw);
  const long pf = i / hw;  // pl * frames + f
  const int f = (int)(pf % frames);
  const unsigned s = (unsigned)map[(long)f * hw + pix];
  half_t v = (half_t)0.0f;
  if (s < (unsigned)hw) v = src[pf * hw + s];
  dst[i] = v;
}

}  // namespace

// run_entry / move_planes (pnp_blend.h) on the WARPED form: the _resampled contract (the _sel contract + a device table) with the
// 2-D map in place of the per-axis maps, and the form's limit on height * width
extern "C" int mvoc_pnp_blend_scatter_tokens_warped(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                    uint32_t active, const int32_t* map, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_tokens_warped", "pnp_tokens_warped_kernel", WARPED, prepare_tokens, d, nsrc, obj_chunk, nvar,
                   active, map, stream, [&](auto n, auto, const Launch& l, const PnpArgs& a) {
                     launch(pnp_tokens_warped_kernel<n.value>, l, a, (int)nvar, (unsigned)active, (const int*)map);
                   });
}

extern "C" int mvoc_pnp_blend_scatter_nchw_warped(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                  uint32_t active, const int32_t* map, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_nchw_warped", "pnp_nchw_warped_kernel", WARPED, prepare_nchw, d, nsrc, obj_chunk, nvar, active,
                   map, stream, [&](auto n, auto v, const Launch& l, const PnpArgs& a) {
                     launch(pnp_nchw_warped_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active, (const int*)map);
                   });
}

extern "C" int mvoc_gather_planes_warped_f16(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w,
                                             const int32_t* map, void* stream) {
  return move_planes(WARPED, "gather_planes_warped_kernel", src, dst, nplane, frames, h, w, map, stream,
                     [&](dim3 grid, hipStream_t s, long n) {
                       hipLaunchKernelGGL(gather_planes_warped_kernel, grid, dim3(256), 0, s, (const half_t*)src, (half_t*)dst,
                                          (int)frames, (int)(h * w), (const int*)map, n);
                     });
}
