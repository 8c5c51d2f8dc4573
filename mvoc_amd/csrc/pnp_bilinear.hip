// Bilinear sampling of warped objects at composition time: the blend-scatter family with the TAPS object load.
// Object j of frame f is read at the four pixels a tap table names for every destination pixel and interpolated with fixed-point
// weights q / 256 on a chain of correctly rounded fp16 operations (lerp16_h, three times: top row, bottom row, between them), so
// the chunks hold the bits the unplaced entries write on sources that were interpolated beforehand by the same chain.  The
// kernels are blend_scatter<L, TAPS, true, NOBJ> composed from the pieces of pnp_blend.h exactly as pnp_warp.hip composes its
// MAP2 kernels.  A translation unit of its own: the kernel census of pnp.o, pnp_variants2.o and pnp_warp.o is pinned by tests.
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

// _bilinear: the _warped contract with the tap table in place of the 2-D map.  A tap row / column + 1 is a 16-bit field of word 0
// and 0xffff is kept for "absent": a site with 65 535 rows or columns or more is refused
int fill_bilinear(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active, const void* taps,
                  PnpArgs& a, double& chunks) {
  MVOC_REQUIRE(taps, -1, "pnp bilinear: null tap table");
  if (int rc = fill_variants_sel(d, nsrc, obj_chunk, nvar, active, a, chunks)) return rc;
  MVOC_REQUIRE((long)d->height * d->width < 0x7fffffffL, -2, "pnp bilinear: height * width does not fit an int");
  MVOC_REQUIRE(d->height < 65535 && d->width < 65535, -2,
               "pnp bilinear: height %d or width %d does not fit the 16-bit tap fields (< 65535)", d->height, d->width);
  return 0;
}

double table_bytes(const mvoc_pnp_desc* d) { return 8.0 * d->nobj * d->frames * (double)d->height * d->width; }

}  // namespace

extern "C" int mvoc_pnp_blend_scatter_tokens_bilinear(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                      uint32_t active, const int32_t* taps, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_tokens_bilinear")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  if (int rc = fill_bilinear(d, nsrc, obj_chunk, nvar, active, taps, a, chunks)) return rc;
  if (int rc = prepare_tokens(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks, 1.0, table_bytes(d)));
  dispatch(d->nobj, l.vec, [&](auto n, auto) {
    launch(pnp_tokens_bilinear_kernel<n.value>, l, a, (int)nvar, (unsigned)active, (const int*)taps);
  });
  return mvoc_check_launch("pnp_tokens_bilinear_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_nchw_bilinear(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                    uint32_t active, const int32_t* taps, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_nchw_bilinear")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  if (int rc = fill_bilinear(d, nsrc, obj_chunk, nvar, active, taps, a, chunks)) return rc;
  if (int rc = prepare_nchw(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks, 1.0, table_bytes(d)));
  dispatch(d->nobj, l.vec, [&](auto n, auto v) {
    launch(pnp_nchw_bilinear_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active, (const int*)taps);
  });
  return mvoc_check_launch("pnp_nchw_bilinear_kernel");
}

extern "C" int mvoc_gather_planes_bilinear_f16(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w,
                                               const int32_t* taps, void* stream) {
  MVOC_REQUIRE(src && dst && taps, -1, "gather_planes_bilinear: null operand");
  MVOC_REQUIRE(src != dst, -1, "gather_planes_bilinear: in place (src == dst) is not supported");
  MVOC_REQUIRE(nplane > 0 && frames > 0 && h > 0 && w > 0, -1, "gather_planes_bilinear: bad dims");
  MVOC_REQUIRE((long)h * w < 0x7fffffffL, -2, "gather_planes_bilinear: h * w does not fit an int");
  MVOC_REQUIRE(h < 65535 && w < 65535, -2, "gather_planes_bilinear: h %d or w %d does not fit the 16-bit tap fields (< 65535)", h, w);
  const long n = (long)nplane * frames * h * w;
  const long nblk = (n + 255) / 256;
  MVOC_REQUIRE(nblk < 0x7fffffffL, -2, "gather_planes_bilinear: grid too large");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * n * 2 + 8.0 * frames * (double)h * w);
  hipLaunchKernelGGL(gather_planes_bilinear_kernel, dim3((unsigned)nblk), dim3(256), 0, s, (const half_t*)src, (half_t*)dst,
                     (int)frames, (int)h, (int)w, (const int*)taps, n);
  return mvoc_check_launch("gather_planes_bilinear_kernel");
}
