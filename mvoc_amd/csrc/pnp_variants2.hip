// Per-variant object transforms: the blend-scatter family's per-variant form with the MAP object load.  Variant
// k reads object j of frame f at (ymap_k[py], xmap_k[px]) of ITS index maps with ITS masks, so K scales / mirrors / positions
// compose over one set of source chunks.  The kernels are blend_scatter_per_variant<L, MAP, NOBJ> of pnp_blend.h -- the pieces
// of pnp.hip's _placed_variants kernels (<L, SHIFT, NOBJ>) with the table rule of its _resampled kernels; nothing here is new
// arithmetic, and variant k's chunks hold the bits a single-variant _resampled call with table k and masks k writes.
// A translation unit of its own: the kernel census of pnp.o is pinned by tests.  It holds the two kernels and one call per entry:
// the form's row (RESAMPLED_VARIANTS) and the body of the entries (run_entry) are in pnp_blend.h, as for pnp.hip, pnp_warp.hip and
// pnp_bilinear.hip.
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

}  // namespace

// run_entry (pnp_blend.h) on the RESAMPLED_VARIANTS form: the _placed_variants contract and chunk count with a table of
// per-axis index maps per variant
extern "C" int mvoc_pnp_blend_scatter_tokens_resampled_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                                int32_t nvar, uint32_t active, const int32_t* maps, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_tokens_resampled_variants", "pnp_tokens_resampled_variants_kernel", RESAMPLED_VARIANTS,
                   prepare_tokens, d, nsrc, obj_chunk, nvar, active, maps, stream, [&](auto n, auto, const Launch& l, const PnpArgs& a) {
                     launch(pnp_tokens_resampled_variants_kernel<n.value>, l, a, (int)nvar, (unsigned)active, (const int*)maps);
                   });
}

extern "C" int mvoc_pnp_blend_scatter_nchw_resampled_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                              int32_t nvar, uint32_t active, const int32_t* maps, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_nchw_resampled_variants", "pnp_nchw_resampled_variants_kernel", RESAMPLED_VARIANTS,
                   prepare_nchw, d, nsrc, obj_chunk, nvar, active, maps, stream, [&](auto n, auto v, const Launch& l, const PnpArgs& a) {
                     launch(pnp_nchw_resampled_variants_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active, (const int*)maps);
                   });
}
