// Rotation of objects at composition time: the blend-scatter family with the MAP2 object load.  Object j of
// frame f is read at the source pixel a 2-D index map names for every destination pixel -- a rotation (or any affine map) is not
// separable into the per-axis maps of the _resampled entries.  The kernels are blend_scatter<L, MAP2, SEL, NOBJ> composed from the
// pieces of pnp_blend.h exactly as pnp.hip composes its _resampled kernels (<L, MAP, SEL, NOBJ>): one table load per pixel in
// place of two, the same gather, the same fp16 blend; only values move, so the chunks hold the bits the unplaced entries write on
// sources gathered beforehand.  A translation unit of its own: the kernel census of pnp.o is pinned by tests.
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

// _warped: the _resampled contract (the _sel contract + a device table) with the 2-D map in place of the per-axis maps.  The
// kernels form height * width as an int and a map entry is an int32: a site of 2^31 pixels or more is refused
int fill_warped(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active, const void* map,
                PnpArgs& a, double& chunks) {
  MVOC_REQUIRE(map, -1, "pnp warped: null map table");
  if (int rc = fill_variants_sel(d, nsrc, obj_chunk, nvar, active, a, chunks)) return rc;
  MVOC_REQUIRE((long)d->height * d->width < 0x7fffffffL, -2, "pnp warped: height * width does not fit the int32 map entries");
  return 0;
}

double table_bytes(const mvoc_pnp_desc* d) { return 4.0 * d->nobj * d->frames * (double)d->height * d->width; }

}  // namespace

extern "C" int mvoc_pnp_blend_scatter_tokens_warped(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                    uint32_t active, const int32_t* map, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_tokens_warped")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  if (int rc = fill_warped(d, nsrc, obj_chunk, nvar, active, map, a, chunks)) return rc;
  if (int rc = prepare_tokens(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks, 1.0, table_bytes(d)));
  dispatch(d->nobj, l.vec, [&](auto n, auto) {
    launch(pnp_tokens_warped_kernel<n.value>, l, a, (int)nvar, (unsigned)active, (const int*)map);
  });
  return mvoc_check_launch("pnp_tokens_warped_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_nchw_warped(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                  uint32_t active, const int32_t* map, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_nchw_warped")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  if (int rc = fill_warped(d, nsrc, obj_chunk, nvar, active, map, a, chunks)) return rc;
  if (int rc = prepare_nchw(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks, 1.0, table_bytes(d)));
  dispatch(d->nobj, l.vec, [&](auto n, auto v) {
    launch(pnp_nchw_warped_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active, (const int*)map);
  });
  return mvoc_check_launch("pnp_nchw_warped_kernel");
}

extern "C" int mvoc_gather_planes_warped_f16(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w,
                                             const int32_t* map, void* stream) {
  MVOC_REQUIRE(src && dst && map, -1, "gather_planes_warped: null operand");
  MVOC_REQUIRE(src != dst, -1, "gather_planes_warped: in place (src == dst) is not supported");
  MVOC_REQUIRE(nplane > 0 && frames > 0 && h > 0 && w > 0, -1, "gather_planes_warped: bad dims");
  MVOC_REQUIRE((long)h * w < 0x7fffffffL, -2, "gather_planes_warped: h * w does not fit the int32 map entries");
  const long n = (long)nplane * frames * h * w;
  const long nblk = (n + 255) / 256;
  MVOC_REQUIRE(nblk < 0x7fffffffL, -2, "gather_planes_warped: grid too large");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * n * 2 + 4.0 * frames * (double)h * w);
  hipLaunchKernelGGL(gather_planes_warped_kernel, dim3((unsigned)nblk), dim3(256), 0, s, (const half_t*)src, (half_t*)dst,
                     (int)frames, (int)(h * w), (const int*)map, n);
  return mvoc_check_launch("gather_planes_warped_kernel");
}
