// PnP masked blend + scatter, latent noise fusion and the fused CFG + DDIM step.  All HBM-bound elementwise
// work; every arithmetic op is rounded to fp16 exactly where the reference's eager fp16 op chain rounds, so
// the results are BIT-EXACT against the reference arithmetic (fp32 compute + one rounding per op equals a
// correctly rounded fp16 op: 24 >= 2*11+2 significand bits).
//
// Traffic per injection site (spatial Q/K at the 320-channel level, B=5, F=16, 64x64): read base + 2 objects,
// write 2 destination chunks, for Q and K = 10 x 41.9 MB + masks (1 fp16 per (frame, pixel), never expanded to
// [F,H,W,C]) = 419.6 MB -- the reference moves several times that through rearrange/repeat copies.
//
// The argument block, the pieces of the blend-scatter family, its table forms and the one host body of its variant entries
// (run_entry) and of the plane movers (move_planes) are in pnp_blend.h, shared with pnp_variants2.hip, pnp_warp.hip and
// pnp_bilinear.hip.
#include "pnp_blend.h"

namespace {

// item = (f, p, c8): 8 consecutive channels of one (frame, pixel)
template <bool MAPPED>
__global__ __launch_bounds__(256) void pnp_tokens_kernel(const PnpArgs p) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  half_t* x = p.x[blockIdx.y];
  const int c8n = p.channels >> 3;
  const int c8 = (int)(idx % c8n);
  const long fp = idx / c8n;
  const int hw = p.height * p.width;
  const int f = (int)(fp / hw), px = (int)(fp % hw);
  const int py = px / p.width, pxx = px - py * p.width;
  const int my = nearest_src(py, p.sy, p.mask_h), mx = nearest_src(pxx, p.sx, p.mask_w);
  const long off = (long)f * p.f_stride + (long)px * p.p_stride + c8 * 8;
  const int nchunk = chunk_count<MAPPED>(p);
  const int basec = p.base_chunk0 ? 0 : nchunk - 1;
  const half8_t bv = *reinterpret_cast<const half8_t*>(x + basec * p.chunk_stride + off);
  float inj[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) inj[e] = (float)bv[e];
  for (int j = 0; j < p.nobj; ++j) {
    const float m = (float)p.masks[(((long)j * p.frames + f) * p.mask_h + my) * p.mask_w + mx];
    const half8_t ov = *reinterpret_cast<const half8_t*>(x + obj_chunk<MAPPED>(p, j) * p.chunk_stride + off);
#pragma unroll
    for (int e = 0; e < 8; ++e) inj[e] = blend16(inj[e], (float)ov[e], m);
  }
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (half_t)inj[e];
  if (p.ndst == 2) *reinterpret_cast<half8_t*>(x + (nchunk - 2) * p.chunk_stride + off) = o;
  *reinterpret_cast<half8_t*>(x + (nchunk - 1) * p.chunk_stride + off) = o;
}

// NCHW: x [(nobj+3)*F, C, H, W]; item = (f, c, p8) with VEC consecutive pixels
template <int VEC, bool MAPPED>
__global__ __launch_bounds__(256) void pnp_nchw_kernel(const PnpArgs p) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  half_t* x = p.x[blockIdx.y];
  const int hw = p.height * p.width;
  const int pvn = hw / VEC;
  const int pv = (int)(idx % pvn);
  const long fc = idx / pvn;
  const int f = (int)(fc / p.channels);
  const long off = fc * hw + (long)pv * VEC;  // (f*C + c)*HW + p
  const long chunk = (long)p.frames * p.channels * hw;
  const int nchunk = chunk_count<MAPPED>(p);
  const int basec = p.base_chunk0 ? 0 : nchunk - 1;
  float inj[VEC];
  half_t tmp[VEC];
  if constexpr (VEC == 8) {
    *reinterpret_cast<half8_t*>(tmp) = *reinterpret_cast<const half8_t*>(x + basec * chunk + off);
  } else {
    tmp[0] = x[basec * chunk + off];
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) inj[e] = (float)tmp[e];
  for (int j = 0; j < p.nobj; ++j) {
    if constexpr (VEC == 8) {
      *reinterpret_cast<half8_t*>(tmp) = *reinterpret_cast<const half8_t*>(x + obj_chunk<MAPPED>(p, j) * chunk + off);
    } else {
      tmp[0] = x[obj_chunk<MAPPED>(p, j) * chunk + off];
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int px = pv * VEC + e;
      const int py = px / p.width, pxx = px - py * p.width;
      const int my = nearest_src(py, p.sy, p.mask_h), mx = nearest_src(pxx, p.sx, p.mask_w);
      const float m = (float)p.masks[(((long)j * p.frames + f) * p.mask_h + my) * p.mask_w + mx];
      inj[e] = blend16(inj[e], (float)tmp[e], m);
    }
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) tmp[e] = (half_t)inj[e];
  if constexpr (VEC == 8) {
    if (p.ndst == 2) *reinterpret_cast<half8_t*>(x + (nchunk - 2) * chunk + off) = *reinterpret_cast<half8_t*>(tmp);
    *reinterpret_cast<half8_t*>(x + (nchunk - 1) * chunk + off) = *reinterpret_cast<half8_t*>(tmp);
  } else {
    if (p.ndst == 2) x[(nchunk - 2) * chunk + off] = tmp[0];
    x[(nchunk - 1) * chunk + off] = tmp[0];
  }
}

// ---- the blend-scatter family: K variants over one set of source chunks -------------------------------
// Batch [s_0..s_{nsrc-1}, u_1..u_K, c_1..c_K] (ndst == 1: [s.., c_1..c_K]).  Ten kernels, every one composed from the same
// four pieces:
//   item geometry   Tokens / Nchw<VEC>::init: the work item's frame, pixel(s) and offsets
//   object load     ::load<S>: NOBJ object vectors and their mask values, by the source rule S --
//                     DIRECT  the object at the destination pixel (vector load; the mask as float)
//                     SHIFT   at (py - dfy, px - dfx) of an offset table (placed_src)
//                     MAP     at (ymap[py], xmap[px]) of per-axis index maps (resampled_src)
//                   SHIFT / MAP: where the source pixel lies outside the frame the object is absent, value 0 and mask 0 enter
//                   the arithmetic like any other pair (it is not skipped: a -0.0 base becomes +0.0 as under a zero mask); the
//                   masks are in destination coordinates and sampled at the destination pixel
//   blend           one base vector over the NOBJ objects in object order: blend16 (DIRECT) or blend16_h (SHIFT / MAP)
//   variant scatter blend_scatter: objects loaded ONCE and kept in registers across the variant loop; one blend for every
//                   variant when the base is chunk 0, else per variant on its own cond chunk; ndst stores per variant; SEL =
//                   bit k of `active` clear: variant k's chunks are neither read nor written (wave-uniform, a kernel argument)
// blend_scatter is in pnp_blend.h (pnp_warp.hip composes its MAP2 kernels from it as well);
// blend_scatter_per_variant (pnp_blend.h) is the same pieces with the object load INSIDE the variant loop.
//   _variants = <DIRECT, no SEL>   _variants_sel = <DIRECT, SEL>   _placed = <SHIFT, SEL>   _resampled = <MAP, SEL>
//   _placed_variants = per-variant <SHIFT, SEL>   (_resampled_variants = per-variant <MAP, SEL>: pnp_variants2.hip)
// NOBJ is a template parameter, so the object arrays are indexed by unrolled constants only (a run-time-indexed array would go
// to scratch, see PnpArgs.obj_map).
template <int NOBJ>
__global__ __launch_bounds__(256) void pnp_tokens_variants_kernel(const PnpArgs p, const int nvar) {
  blend_scatter<Tokens, DIRECT, false, NOBJ>(p, nvar, 0u, nullptr);
}

template <int VEC, int NOBJ>
__global__ __launch_bounds__(256) void pnp_nchw_variants_kernel(const PnpArgs p, const int nvar) {
  blend_scatter<Nchw<VEC>, DIRECT, false, NOBJ>(p, nvar, 0u, nullptr);
}

template <int NOBJ>
__global__ __launch_bounds__(256) void pnp_tokens_variants_sel_kernel(const PnpArgs p, const int nvar, const unsigned active) {
  blend_scatter<Tokens, DIRECT, true, NOBJ>(p, nvar, active, nullptr);
}

template <int VEC, int NOBJ>
__global__ __launch_bounds__(256) void pnp_nchw_variants_sel_kernel(const PnpArgs p, const int nvar, const unsigned active) {
  blend_scatter<Nchw<VEC>, DIRECT, true, NOBJ>(p, nvar, active, nullptr);
}

template <int NOBJ>
__global__ __launch_bounds__(256) void pnp_tokens_placed_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                                const int* __restrict__ place) {
  blend_scatter<Tokens, SHIFT, true, NOBJ>(p, nvar, active, place);
}

template <int VEC, int NOBJ>
__global__ __launch_bounds__(256) void pnp_nchw_placed_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                              const int* __restrict__ place) {
  blend_scatter<Nchw<VEC>, SHIFT, true, NOBJ>(p, nvar, active, place);
}

template <int NOBJ>
__global__ __launch_bounds__(256) void pnp_tokens_placed_variants_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                                         const int* __restrict__ place) {
  blend_scatter_per_variant<Tokens, SHIFT, NOBJ>(p, nvar, active, place);
}

template <int VEC, int NOBJ>
__global__ __launch_bounds__(256) void pnp_nchw_placed_variants_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                                       const int* __restrict__ place) {
  blend_scatter_per_variant<Nchw<VEC>, SHIFT, NOBJ>(p, nvar, active, place);
}

template <int NOBJ>
__global__ __launch_bounds__(256) void pnp_tokens_resampled_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                                   const int* __restrict__ maps) {
  blend_scatter<Tokens, MAP, true, NOBJ>(p, nvar, active, maps);
}

template <int VEC, int NOBJ>
__global__ __launch_bounds__(256) void pnp_nchw_resampled_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                                 const int* __restrict__ maps) {
  blend_scatter<Nchw<VEC>, MAP, true, NOBJ>(p, nvar, active, maps);
}

// zero-filled per-frame gather of [nplane][F][h][w]: dst[pl, f, y, x] = src[pl, f, ymap_f[y], xmap_f[x]] or 0 where either
// index is outside the plane (compared unsigned: every int32 entry is safe); maps = F rows of h + w int32 (ymap, then xmap) on
// the device, shared by the planes
__global__ __launch_bounds__(256) void gather_planes_kernel(const half_t* __restrict__ src, half_t* __restrict__ dst, int frames,
                                                            int h, int w, const int* __restrict__ maps, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int xx = (int)(i % w);
  const long r = i / w;
  const int y = (int)(r % h);
  const long pf = r / h;  // pl * frames + f
  const int f = (int)(pf % frames);
  const int* mp = maps + (long)f * ((long)h + w);
  const unsigned sy = (unsigned)mp[y], sx = (unsigned)mp[h + xx];
  half_t v = (half_t)0.0f;
  if (sy < (unsigned)h && sx < (unsigned)w) v = src[(pf * h + sy) * w + sx];
  dst[i] = v;
}

// zero-filled per-frame integer translation of [nplane][F][h][w]: dst[pl, f, y, x] = src[pl, f, y - dy_f, x - dx_f] or 0;
// offsets = F int32 pairs (dy_f, dx_f) on the device, shared by the planes
__global__ __launch_bounds__(256) void shift_planes_kernel(const half_t* __restrict__ src, half_t* __restrict__ dst, int frames,
                                                           int h, int w, const int* __restrict__ offsets, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int xx = (int)(i % w);
  const long r = i / w;
  const int y = (int)(r % h);
  const long pf = r / h;  // pl * frames + f
  const int f = (int)(pf % frames);
  const long sy = (long)y - offsets[2 * f], sx = (long)xx - offsets[2 * f + 1];
  half_t v = (half_t)0.0f;
  if (sy >= 0 && sy < h && sx >= 0 && sx < w) v = src[(pf * h + sy) * w + sx];
  dst[i] = v;
}

// ---- loop glue -----------------------------------------------------------------------------------
// fp32-scalar x fp16-tensor products of the reference's eager chain (python float / 0-dim fp32 tensor times a
// half tensor) are formed in fp32, ROUNDED TO fp32, then rounded to fp16 -- two roundings.  Left to itself hipcc
// contracts `(half)(s * (float)h)` into v_fma_mixlo_f16, which rounds the exact 35-bit product once and differs
// by 1 ulp at ~2^-9 of the elements (observed on MI355X).  The empty asm pins the fp32 product in a VGPR.
__device__ __forceinline__ float smul16(float scalar, float x) {
  float p = scalar * x;
  asm volatile("" : "+v"(p));
  return r16(p);
}

__global__ __launch_bounds__(256) void ddim_step_kernel(const half_t* __restrict__ x, const half_t* __restrict__ vu,
                                                        const half_t* __restrict__ vc, const float* __restrict__ coef,
                                                        half_t* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float sa = coef[0], sb = coef[1], sp = coef[2], sq = coef[3], g = coef[4];
  const float xs = (float)x[i];
  float v = (float)vc[i];
  if (vu) {
    const float u = (float)vu[i];
    v = r16(u + smul16(g, r16(v - u)));
  }
  const float x0 = r16(smul16(sa, xs) - smul16(sb, v));
  const float eps = r16(smul16(sa, v) + smul16(sb, xs));
  const float dir = smul16(sq, eps);
  out[i] = (half_t)(smul16(sp, x0) + dir);
}

__global__ __launch_bounds__(256) void fusion_kernel(const half_t* __restrict__ lat, const half_t* __restrict__ bg,
                                                     const half_t* __restrict__ objs, const half_t* __restrict__ masks,
                                                     half_t* __restrict__ out, int nobj, long n, float mix, float omix,
                                                     int rnf) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float l = r16(smul16(mix, (float)lat[i]) + smul16(omix, (float)bg[i]));
  for (int j = 0; j < nobj; ++j) {
    const float m = (float)masks[(long)j * n + i];
    const float inv_obj = r16((float)objs[(long)j * n + i] * m);
    const float background = r16(l * r16(1.0f - m));
    float fusion = inv_obj;
    if (rnf) fusion = r16(smul16(mix, r16(l * m)) + smul16(omix, inv_obj));
    l = r16(background + fusion);
  }
  out[i] = (half_t)l;
}

// K variants: element i belongs to variant i / n_per and takes that variant's coefficient row; the arithmetic is
// ddim_step_kernel's, operation for operation
__global__ __launch_bounds__(256) void ddim_step_variants_kernel(const half_t* __restrict__ x, const half_t* __restrict__ vu,
                                                                 const half_t* __restrict__ vc, const float* __restrict__ coef,
                                                                 half_t* __restrict__ out, long n_per, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* cf = coef + 5 * (i / n_per);
  const float sa = cf[0], sb = cf[1], sp = cf[2], sq = cf[3], g = cf[4];
  const float xs = (float)x[i];
  float v = (float)vc[i];
  if (vu) {
    const float u = (float)vu[i];
    v = r16(u + smul16(g, r16(v - u)));
  }
  const float x0 = r16(smul16(sa, xs) - smul16(sb, v));
  const float eps = r16(smul16(sa, v) + smul16(sb, xs));
  const float dir = smul16(sq, eps);
  out[i] = (half_t)(smul16(sp, x0) + dir);
}

// K variants: latents / out are [nvar][n_per]; background, objects and masks are [n_per] and read by every variant
__global__ __launch_bounds__(256) void fusion_variants_kernel(const half_t* __restrict__ lat, const half_t* __restrict__ bg,
                                                              const half_t* __restrict__ objs, const half_t* __restrict__ masks,
                                                              half_t* __restrict__ out, int nobj, long n_per, long n, float mix,
                                                              float omix, int rnf) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long r = i % n_per;
  float l = r16(smul16(mix, (float)lat[i]) + smul16(omix, (float)bg[r]));
  for (int j = 0; j < nobj; ++j) {
    const float m = (float)masks[(long)j * n_per + r];
    const float inv_obj = r16((float)objs[(long)j * n_per + r] * m);
    const float background = r16(l * r16(1.0f - m));
    float fusion = inv_obj;
    if (rnf) fusion = r16(smul16(mix, r16(l * m)) + smul16(omix, inv_obj));
    l = r16(background + fusion);
  }
  out[i] = (half_t)l;
}

// nread: source chunks read from HBM (the base included); ndst chunks written
template <bool MAPPED>
int launch_tokens(const mvoc_pnp_desc* d, PnpArgs& a, int nread, void* stream) {
  Launch l;
  if (int rc = prepare_tokens(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, nread + a.ndst));
  launch(pnp_tokens_kernel<MAPPED>, l, a);
  return mvoc_check_launch("pnp_tokens_kernel");
}

template <bool MAPPED>
int launch_nchw(const mvoc_pnp_desc* d, PnpArgs& a, int nread, void* stream) {
  Launch l;
  if (int rc = prepare_nchw(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, nread + a.ndst));
  if (l.vec) launch(pnp_nchw_kernel<8, MAPPED>, l, a);
  else launch(pnp_nchw_kernel<1, MAPPED>, l, a);
  return mvoc_check_launch("pnp_nchw_kernel");
}

}  // namespace

// Every entry below is run_entry (pnp_blend.h) on its table form, its layout's prepare_* and the launch of its own kernel.
extern "C" int mvoc_pnp_blend_scatter_tokens_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                      int32_t nvar, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_tokens_variants", "pnp_tokens_variants_kernel", NO_TABLE, prepare_tokens, d, nsrc, obj_chunk,
                   nvar, all_variants(nvar), nullptr, stream, [&](auto n, auto, const Launch& l, const PnpArgs& a) {
                     launch(pnp_tokens_variants_kernel<n.value>, l, a, (int)nvar);
                   });
}

extern "C" int mvoc_pnp_blend_scatter_nchw_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                    int32_t nvar, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_nchw_variants", "pnp_nchw_variants_kernel", NO_TABLE, prepare_nchw, d, nsrc, obj_chunk, nvar,
                   all_variants(nvar), nullptr, stream, [&](auto n, auto v, const Launch& l, const PnpArgs& a) {
                     launch(pnp_nchw_variants_kernel<v.value, n.value>, l, a, (int)nvar);
                   });
}

extern "C" int mvoc_pnp_blend_scatter_tokens_variants_sel(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                          int32_t nvar, uint32_t active, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_tokens_variants_sel", "pnp_tokens_variants_sel_kernel", NO_TABLE, prepare_tokens, d, nsrc,
                   obj_chunk, nvar, active, nullptr, stream, [&](auto n, auto, const Launch& l, const PnpArgs& a) {
                     launch(pnp_tokens_variants_sel_kernel<n.value>, l, a, (int)nvar, (unsigned)active);
                   });
}

extern "C" int mvoc_pnp_blend_scatter_nchw_variants_sel(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                        int32_t nvar, uint32_t active, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_nchw_variants_sel", "pnp_nchw_variants_sel_kernel", NO_TABLE, prepare_nchw, d, nsrc, obj_chunk,
                   nvar, active, nullptr, stream, [&](auto n, auto v, const Launch& l, const PnpArgs& a) {
                     launch(pnp_nchw_variants_sel_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active);
                   });
}

extern "C" int mvoc_pnp_blend_scatter_tokens_placed(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                    uint32_t active, const int32_t* place, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_tokens_placed", "pnp_tokens_placed_kernel", PLACED, prepare_tokens, d, nsrc, obj_chunk, nvar,
                   active, place, stream, [&](auto n, auto, const Launch& l, const PnpArgs& a) {
                     launch(pnp_tokens_placed_kernel<n.value>, l, a, (int)nvar, (unsigned)active, (const int*)place);
                   });
}

extern "C" int mvoc_pnp_blend_scatter_nchw_placed(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                  uint32_t active, const int32_t* place, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_nchw_placed", "pnp_nchw_placed_kernel", PLACED, prepare_nchw, d, nsrc, obj_chunk, nvar, active,
                   place, stream, [&](auto n, auto v, const Launch& l, const PnpArgs& a) {
                     launch(pnp_nchw_placed_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active, (const int*)place);
                   });
}

extern "C" int mvoc_pnp_blend_scatter_tokens_placed_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                             int32_t nvar, uint32_t active, const int32_t* place, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_tokens_placed_variants", "pnp_tokens_placed_variants_kernel", PLACED_VARIANTS, prepare_tokens,
                   d, nsrc, obj_chunk, nvar, active, place, stream, [&](auto n, auto, const Launch& l, const PnpArgs& a) {
                     launch(pnp_tokens_placed_variants_kernel<n.value>, l, a, (int)nvar, (unsigned)active, (const int*)place);
                   });
}

extern "C" int mvoc_pnp_blend_scatter_nchw_placed_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                           int32_t nvar, uint32_t active, const int32_t* place, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_nchw_placed_variants", "pnp_nchw_placed_variants_kernel", PLACED_VARIANTS, prepare_nchw, d,
                   nsrc, obj_chunk, nvar, active, place, stream, [&](auto n, auto v, const Launch& l, const PnpArgs& a) {
                     launch(pnp_nchw_placed_variants_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active, (const int*)place);
                   });
}

extern "C" int mvoc_pnp_blend_scatter_tokens_resampled(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                       uint32_t active, const int32_t* maps, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_tokens_resampled", "pnp_tokens_resampled_kernel", RESAMPLED, prepare_tokens, d, nsrc,
                   obj_chunk, nvar, active, maps, stream, [&](auto n, auto, const Launch& l, const PnpArgs& a) {
                     launch(pnp_tokens_resampled_kernel<n.value>, l, a, (int)nvar, (unsigned)active, (const int*)maps);
                   });
}

extern "C" int mvoc_pnp_blend_scatter_nchw_resampled(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                     uint32_t active, const int32_t* maps, void* stream) {
  return run_entry("mvoc_pnp_blend_scatter_nchw_resampled", "pnp_nchw_resampled_kernel", RESAMPLED, prepare_nchw, d, nsrc, obj_chunk,
                   nvar, active, maps, stream, [&](auto n, auto v, const Launch& l, const PnpArgs& a) {
                     launch(pnp_nchw_resampled_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active, (const int*)maps);
                   });
}

extern "C" int mvoc_gather_planes_f16(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w,
                                      const int32_t* maps, void* stream) {
  return move_planes(RESAMPLED, "gather_planes_kernel", src, dst, nplane, frames, h, w, maps, stream, [&](dim3 grid, hipStream_t s, long n) {
    hipLaunchKernelGGL(gather_planes_kernel, grid, dim3(256), 0, s, (const half_t*)src, (half_t*)dst, (int)frames, (int)h, (int)w,
                       (const int*)maps, n);
  });
}

extern "C" int mvoc_shift_planes_f16(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w,
                                     const int32_t* offsets, void* stream) {
  return move_planes(PLACED, "shift_planes_kernel", src, dst, nplane, frames, h, w, offsets, stream, [&](dim3 grid, hipStream_t s, long n) {
    hipLaunchKernelGGL(shift_planes_kernel, grid, dim3(256), 0, s, (const half_t*)src, (half_t*)dst, (int)frames, (int)h, (int)w,
                       (const int*)offsets, n);
  });
}

extern "C" int mvoc_ddim_step_variants_f16(const void* x, const void* v_uncond, const void* v_cond, const float* coef_dev,
                                           void* out, int64_t n_per, int32_t nvar, void* stream) {
  MVOC_REQUIRE(x && v_cond && coef_dev && out && n_per > 0, -1, "ddim_step_variants: null operand / empty");
  MVOC_REQUIRE(nvar >= 1 && nvar <= 8, -1, "ddim_step_variants: nvar %d not in [1, 8]", nvar);
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)n_per * nvar;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * n * (v_uncond ? 4 : 3));
  hipLaunchKernelGGL(ddim_step_variants_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const half_t*)x,
                     (const half_t*)v_uncond, (const half_t*)v_cond, coef_dev, (half_t*)out, (long)n_per, n);
  return mvoc_check_launch("ddim_step_variants_kernel");
}

extern "C" int mvoc_latent_fusion_variants_f16(const void* latents, const void* bg, const void* objs, const void* masks,
                                               void* out, int32_t nobj, int64_t n_per, int32_t nvar, double mix_ratio,
                                               int32_t obj_random_noise_fusion, void* stream) {
  MVOC_REQUIRE(latents && bg && objs && masks && out && n_per > 0 && nobj >= 0, -1, "latent_fusion_variants: null operand / empty");
  MVOC_REQUIRE(nvar >= 1 && nvar <= 8, -1, "latent_fusion_variants: nvar %d not in [1, 8]", nvar);
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)n_per * nvar;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * n * 2 + 2.0 * n_per * (1 + 2 * nobj));
  const float mix = (float)mix_ratio, omix = (float)(1.0 - mix_ratio);  // as mvoc_latent_fusion_f16 forms them
  hipLaunchKernelGGL(fusion_variants_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const half_t*)latents,
                     (const half_t*)bg, (const half_t*)objs, (const half_t*)masks, (half_t*)out, nobj, (long)n_per, n, mix, omix,
                     obj_random_noise_fusion);
  return mvoc_check_launch("fusion_variants_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_tokens(const mvoc_pnp_desc* d, void* stream) {
  PnpArgs a;
  if (int rc = fill_args(d, a)) return rc;
  if (d->base_chunk0 == -1) {  // no background chunk: the base is the last chunk, as with base_chunk0 = 0
    a.no_background = 1;
    a.base_chunk0 = 0;
  }
  // chunks read: nobj objects + the base (chunk 0, or the last chunk) -- the same count in both layouts
  return launch_tokens<false>(d, a, d->nobj + 1, stream);
}

extern "C" int mvoc_pnp_blend_scatter_nchw(const mvoc_pnp_desc* d, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_nchw")) return rc;
  PnpArgs a;
  if (int rc = fill_args(d, a)) return rc;
  return launch_nchw<false>(d, a, d->nobj + 1, stream);
}

extern "C" int mvoc_pnp_blend_scatter_tokens_mapped(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                    void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_tokens_mapped")) return rc;
  PnpArgs a;
  int nread = 0;
  if (int rc = fill_args(d, a)) return rc;
  if (int rc = fill_map(d, nsrc, obj_chunk, a, nread)) return rc;
  return launch_tokens<true>(d, a, nread, stream);
}

extern "C" int mvoc_pnp_blend_scatter_nchw_mapped(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                  void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_nchw_mapped")) return rc;
  PnpArgs a;
  int nread = 0;
  if (int rc = fill_args(d, a)) return rc;
  if (int rc = fill_map(d, nsrc, obj_chunk, a, nread)) return rc;
  return launch_nchw<true>(d, a, nread, stream);
}

extern "C" int mvoc_ddim_step_f16(const void* x, const void* v_uncond, const void* v_cond, const float* coef_dev,
                                  void* out, int64_t n, void* stream) {
  MVOC_REQUIRE(x && v_cond && coef_dev && out && n > 0, -1, "ddim_step: null operand / empty");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * n * (v_uncond ? 4 : 3));
  hipLaunchKernelGGL(ddim_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const half_t*)x,
                     (const half_t*)v_uncond, (const half_t*)v_cond, coef_dev, (half_t*)out, (long)n);
  return mvoc_check_launch("ddim_step_kernel");
}

extern "C" int mvoc_latent_fusion_f16(const void* latents, const void* bg, const void* objs, const void* masks, void* out,
                                      int32_t nobj, int64_t n, double mix_ratio, int32_t obj_random_noise_fusion,
                                      void* stream) {
  MVOC_REQUIRE(latents && bg && objs && masks && out && n > 0 && nobj >= 0, -1, "latent_fusion: null operand / empty");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * n * (3 + 2 * nobj));
  // python-float factors of the reference: mix_ratio and (1.0 - mix_ratio) are formed in double, used as fp32
  const float mix = (float)mix_ratio, omix = (float)(1.0 - mix_ratio);
  hipLaunchKernelGGL(fusion_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const half_t*)latents,
                     (const half_t*)bg, (const half_t*)objs, (const half_t*)masks, (half_t*)out, nobj, (long)n, mix, omix,
                     obj_random_noise_fusion);
  return mvoc_check_launch("fusion_kernel");
}
