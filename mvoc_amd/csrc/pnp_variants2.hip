// Per-variant object transforms: the blend-scatter family's per-variant form with the MAP object load.  Variant
// k reads object j of frame f at (ymap_k[py], xmap_k[px]) of ITS index maps with ITS masks, so K scales / mirrors / positions
// compose over one set of source chunks.  The kernels are blend_scatter_per_variant<L, MAP, NOBJ> of pnp_blend.h -- the pieces
// of pnp.hip's _placed_variants kernels (<L, SHIFT, NOBJ>) with the table rule of its _resampled kernels; nothing here is new
// arithmetic, and variant k's chunks hold the bits a single-variant _resampled call with table k and masks k writes.
// A translation unit of its own: the kernel census of pnp.o is pinned by tests.
#include "pnp_blend.h"

namespace {

template <int NOBJ>
__global__ __launch_bounds__(256) void pnp_tokens_resampled_variants_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                                            const int* __restrict__ maps) {
  blend_scatter_per_variant<Tokens, MAP, NOBJ>(p, nvar, active, maps);
}

template <int VEC, int NOBJ>
__global__ __launch_bounds__(256) void pnp_nchw_resampled_variants_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                                          const int* __restrict__ maps) {
  blend_scatter_per_variant<Nchw<VEC>, MAP, NOBJ>(p, nvar, active, maps);
}

// the _placed_variants contract and chunk count with a table of per-axis index maps per variant
int fill_resampled_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active,
                            const void* maps, PnpArgs& a, double& chunks, int& on) {
  MVOC_REQUIRE(maps, -1, "pnp resampled variants: null map table");
  return fill_placed_variants(d, nsrc, obj_chunk, nvar, active, maps, a, chunks, on);
}

double table_bytes(const mvoc_pnp_desc* d, int32_t nvar) {
  return 4.0 * nvar * d->nobj * d->frames * ((double)d->height + d->width);
}

}  // namespace

extern "C" int mvoc_pnp_blend_scatter_tokens_resampled_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                                int32_t nvar, uint32_t active, const int32_t* maps, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_tokens_resampled_variants")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  int on = 0;
  if (int rc = fill_resampled_variants(d, nsrc, obj_chunk, nvar, active, maps, a, chunks, on)) return rc;
  if (int rc = prepare_tokens(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks, on, table_bytes(d, nvar)));
  dispatch(d->nobj, l.vec, [&](auto n, auto) {
    launch(pnp_tokens_resampled_variants_kernel<n.value>, l, a, (int)nvar, (unsigned)active, (const int*)maps);
  });
  return mvoc_check_launch("pnp_tokens_resampled_variants_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_nchw_resampled_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                              int32_t nvar, uint32_t active, const int32_t* maps, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_nchw_resampled_variants")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  int on = 0;
  if (int rc = fill_resampled_variants(d, nsrc, obj_chunk, nvar, active, maps, a, chunks, on)) return rc;
  if (int rc = prepare_nchw(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks, on, table_bytes(d, nvar)));
  dispatch(d->nobj, l.vec, [&](auto n, auto v) {
    launch(pnp_nchw_resampled_variants_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active, (const int*)maps);
  });
  return mvoc_check_launch("pnp_nchw_resampled_variants_kernel");
}
