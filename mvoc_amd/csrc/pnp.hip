// PnP masked blend + scatter, latent noise fusion and the fused CFG + DDIM step.  All HBM-bound elementwise
// work; every arithmetic op is rounded to fp16 exactly where the reference's eager fp16 op chain rounds, so
// the results are BIT-EXACT against the reference arithmetic (fp32 compute + one rounding per op equals a
// correctly rounded fp16 op: 24 >= 2*11+2 significand bits).
//
// Traffic per injection site (spatial Q/K at the 320-channel level, B=5, F=16, 64x64): read base + 2 objects,
// write 2 destination chunks, for Q and K = 10 x 41.9 MB + masks (1 fp16 per (frame, pixel), never expanded to
// [F,H,W,C]) = 419.6 MB -- the reference moves several times that through rearrange/repeat copies.
#include <type_traits>

#include "common.h"

namespace {

struct PnpArgs {
  half_t* x[2];
  const half_t* masks;
  long chunk_stride, f_stride, p_stride;
  int nobj, frames, height, width, channels, mask_h, mask_w, base_chunk0;
  int ndst;      // trailing destination chunks: 2 = [uncond, cond] (the reference's CFG layout), 1 = [cond] (CFG off)
  float sy, sx;  // nearest-resize scales mask_h/height, mask_w/width (as F.interpolate computes them)
  long total;    // work items per tensor
  // (MAPPED kernels) source de-duplication: chunks 0..nsrc-1 are sources, object j reads chunk (obj_map >> 4j) & 15.  A packed
  // scalar, not an array: the run-time object loop indexes it with a shift (a run-time-indexed array member risks scratch)
  int nsrc;
  unsigned obj_map;
  // (positional kernels) 1: the batch has no background chunk, [obj_1..obj_n, (uncond,) cond] -- object j is chunk j, the base
  // the last chunk (mvoc_pnp_desc.base_chunk0 = -1; base_chunk0 is 0 here)
  int no_background;
};

template <bool MAPPED>
__device__ __forceinline__ int obj_chunk(const PnpArgs& p, int j) {
  if constexpr (MAPPED) return (int)((p.obj_map >> (4 * j)) & 15u);
  return p.no_background ? j : j + 1;
}

template <bool MAPPED>
__device__ __forceinline__ int chunk_count(const PnpArgs& p) {
  if constexpr (MAPPED) return p.nsrc + p.ndst;
  return p.nobj + (p.no_background ? 0 : 1) + p.ndst;
}

__device__ __forceinline__ float blend16(float inj, float obj, float m) {
  const float om = r16(1.0f - m);
  return r16(r16(inj * om) + r16(obj * m));
}

__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) {
  return min((int)floorf(dst * scale), in_size - 1);
}

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
// blend_scatter_per_variant is the same pieces with the object load INSIDE the variant loop.
//   _variants = <DIRECT, no SEL>   _variants_sel = <DIRECT, SEL>   _placed = <SHIFT, SEL>   _resampled = <MAP, SEL>
//   _placed_variants = per-variant <SHIFT, SEL>
// NOBJ is a template parameter, so the object arrays are indexed by unrolled constants only (a run-time-indexed array would go
// to scratch, see PnpArgs.obj_map).
__device__ __forceinline__ int var_dst(const PnpArgs& p, int nvar, int d, int k) {  // d: 0 = first block of destinations
  return p.nsrc + d * nvar + k;
}

template <int VEC>
__device__ __forceinline__ void ld_vec(half_t (&t)[VEC], const half_t* src) {
  if constexpr (VEC == 8) *reinterpret_cast<half8_t*>(t) = *reinterpret_cast<const half8_t*>(src);
  else t[0] = src[0];
}

template <int VEC>
__device__ __forceinline__ void st_vec(half_t* dst, const half_t (&t)[VEC]) {
  if constexpr (VEC == 8) *reinterpret_cast<half8_t*>(dst) = *reinterpret_cast<const half8_t*>(t);
  else dst[0] = t[0];
}

// blend16 on fp16 operands, one correctly rounded fp16 operation per statement (the same values as blend16: each of its float
// operations on fp16 inputs is rounded to fp16 at once).  The SHIFT / MAP loads SELECT their object value and mask (absent: 0, 0), and
// with float operands behind a select hipcc forms r16(obj * m) as a mixed-precision fma with a +0.0 addend, which turns a -0.0
// product into +0.0 -- the DIRECT kernels multiply in fp16 and keep it.  Written in fp16, no such choice is left to the compiler.
__device__ __forceinline__ half_t blend16_h(half_t inj, half_t obj, half_t m) {
  const half_t om = (half_t)1.0f - m;
  const half_t a = inj * om;
  const half_t b = obj * m;
  return a + b;
}

// SHIFT: place = int32 [nobj][frames][2], (dfy, dfx) of object j in frame f -- a device table for THIS site's H x W, constant
// for the whole call
__device__ __forceinline__ bool placed_src(const int* __restrict__ place, int j, int frames, int f, int py, int px, int h, int w,
                                           long& spix) {
  const int* o = place + ((long)j * frames + f) * 2;
  const long sy = (long)py - o[0], sx = (long)px - o[1];  // 64-bit: every int32 offset is safe
  spix = sy * w + sx;
  return sy >= 0 && sy < h && sx >= 0 && sx < w;
}

// MAP: maps = int32 [nobj][frames][height + width] (ymap first, then xmap) -- a device table for THIS site's H x W, constant for
// the whole call.  The kernels cannot see who wrote the table: an entry is compared UNSIGNED against height / width, anything
// outside (every negative value included) means the object is absent there, and the source pixel is formed in 64 bits.
__device__ __forceinline__ bool resampled_src(const int* __restrict__ maps, int j, int frames, int f, int py, int px, int h, int w,
                                              long& spix) {
  const int* mp = maps + ((long)j * frames + f) * ((long)h + w);
  const unsigned sy = (unsigned)mp[py], sx = (unsigned)mp[h + px];
  spix = (long)sy * w + sx;
  return sy < (unsigned)h && sx < (unsigned)w;
}

enum Src { DIRECT, SHIFT, MAP };

template <Src S>
__device__ __forceinline__ bool obj_src(const int* __restrict__ tab, int j, int frames, int f, int py, int px, int h, int w,
                                        long& spix) {
  if constexpr (S == SHIFT) return placed_src(tab, j, frames, f, py, px, h, w, spix);
  else return resampled_src(tab, j, frames, f, py, px, h, w, spix);
}

// NOBJ object vectors of W elements with NM mask values each (tokens: one pixel, NM = 1; NCHW: one per pixel)
template <Src S, int NOBJ, int W, int NM>
struct Objs {
  half_t v[NOBJ][W];
  std::conditional_t<S == DIRECT, float, half_t> m[NOBJ][NM];
};

template <Src S, int NOBJ, int W, int NM>
__device__ __forceinline__ void blend(const half_t (&base)[W], const Objs<S, NOBJ, W, NM>& o, half_t (&out)[W]) {
#pragma unroll
  for (int e = 0; e < W; ++e) {
    if constexpr (S == DIRECT) {
      float inj = (float)base[e];
#pragma unroll
      for (int j = 0; j < NOBJ; ++j) inj = blend16(inj, (float)o.v[j][e], o.m[j][NM == 1 ? 0 : e]);
      out[e] = (half_t)inj;
    } else {
      half_t inj = base[e];
#pragma unroll
      for (int j = 0; j < NOBJ; ++j) inj = blend16_h(inj, o.v[j][e], o.m[j][NM == 1 ? 0 : e]);
      out[e] = inj;
    }
  }
}

__device__ __forceinline__ long mask_index(const PnpArgs& p, int j, int f, int my, int mx) {
  return (((long)j * p.frames + f) * p.mask_h + my) * p.mask_w + mx;
}

// tokens: item = (f, p, c8), 8 consecutive channels of one (frame, pixel)
struct Tokens {
  static constexpr int W = 8, NM = 1;
  int f, py, px, my, mx;
  long foff, off, chunk;  // foff: the item's frame and channels, off: + its pixel; chunk stride

  __device__ __forceinline__ bool init(const PnpArgs& p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total) return false;
    const int c8n = p.channels >> 3;
    const int c8 = (int)(idx % c8n);
    const long fp = idx / c8n;
    const int hw = p.height * p.width;
    f = (int)(fp / hw);
    const int pix = (int)(fp % hw);
    py = pix / p.width, px = pix - py * p.width;
    my = nearest_src(py, p.sy, p.mask_h), mx = nearest_src(px, p.sx, p.mask_w);
    foff = (long)f * p.f_stride + c8 * 8;
    off = foff + (long)pix * p.p_stride;
    chunk = p.chunk_stride;
    return true;
  }

  __device__ __forceinline__ Tokens per_variant() const { return *this; }

  template <Src S, int NOBJ>
  __device__ __forceinline__ void load(const PnpArgs& p, const half_t* x, const half_t* masks, const int* __restrict__ tab,
                                       Objs<S, NOBJ, 8, 1>& o) const {
#pragma unroll
    for (int j = 0; j < NOBJ; ++j) {
      const half_t* src = x + obj_chunk<true>(p, j) * chunk;
      if constexpr (S == DIRECT) {
        o.m[j][0] = (float)masks[mask_index(p, j, f, my, mx)];
        ld_vec<8>(o.v[j], src + off);
      } else {
        long spix;
        const bool in = obj_src<S>(tab, j, p.frames, f, py, px, p.height, p.width, spix);
        o.m[j][0] = (half_t)0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.v[j][e] = (half_t)0.0f;
        if (in) {
          o.m[j][0] = masks[mask_index(p, j, f, my, mx)];
          ld_vec<8>(o.v[j], src + foff + spix * p.p_stride);
        }
      }
    }
  }
};

// NCHW: x [chunks * F, C, H, W]; item = (f, c, pv) with VEC consecutive pixels.  SHIFT / MAP read the object values one pixel at
// a time: a shift in x breaks the 8-pixel alignment of the object rows and under a scale neighbouring destinations no longer read
// neighbouring sources, so each of the VEC pixels has its own source pixel; the base and the destinations keep the vector accesses
template <int VEC>
struct Nchw {
  static constexpr int W = VEC, NM = VEC;
  int f, pv;
  long plane, off, chunk;  // plane: (f*C + c)*HW, off: + the item's first pixel; chunk stride

  __device__ __forceinline__ bool init(const PnpArgs& p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total) return false;
    const int hw = p.height * p.width;
    const int pvn = hw / VEC;
    pv = (int)(idx % pvn);
    const long fc = idx / pvn;
    f = (int)(fc / p.channels);
    plane = fc * hw;
    off = plane + (long)pv * VEC;
    chunk = (long)p.frames * p.channels * hw;
    return true;
  }

  // The per-pixel terms of a load (row / column, mask index, 64-bit bases) do not depend on the variant; hoisted out of the
  // variant loop of blend_scatter_per_variant they stay live across it (202 VGPRs at NOBJ = 4, VEC = 8).  The empty asm makes
  // pv opaque per iteration, so they are formed inside the loop like the object values (154).
  __device__ __forceinline__ Nchw per_variant() const {
    Nchw it = *this;
    asm volatile("" : "+v"(it.pv));
    return it;
  }

  template <Src S, int NOBJ>
  __device__ __forceinline__ void load(const PnpArgs& p, const half_t* x, const half_t* masks, const int* __restrict__ tab,
                                       Objs<S, NOBJ, VEC, VEC>& o) const {
    if constexpr (S == DIRECT) {
      // The pixels' offsets inside one mask plane are formed ONCE, outside the object loop, and object j adds its plane: left
      // inside, hipcc forms the whole 64-bit index per (object, pixel) and the <8, 2..4> instantiations sit at or above their
      // occupancy steps (64 / 64 / 80 VGPRs and more); this way they need 46 / 60 / 66.  The masks are read before the vector.
      long mpix[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const int pix = pv * VEC + e;
        const int py = pix / p.width, px = pix - py * p.width;
        mpix[e] = (long)nearest_src(py, p.sy, p.mask_h) * p.mask_w + nearest_src(px, p.sx, p.mask_w);
      }
#pragma unroll
      for (int j = 0; j < NOBJ; ++j) {
        const half_t* mj = masks + ((long)j * p.frames + f) * ((long)p.mask_h * p.mask_w);
#pragma unroll
        for (int e = 0; e < VEC; ++e) o.m[j][e] = (float)mj[mpix[e]];
        ld_vec<VEC>(o.v[j], x + obj_chunk<true>(p, j) * chunk + off);
      }
    } else {
#pragma unroll
      for (int j = 0; j < NOBJ; ++j) {
        const half_t* src = x + obj_chunk<true>(p, j) * chunk + plane;
        const long mrow = ((long)j * p.frames + f) * p.mask_h;  // first mask row of (object, frame)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const int pix = pv * VEC + e;
          const int py = pix / p.width, px = pix - py * p.width;
          long spix;
          const bool in = obj_src<S>(tab, j, p.frames, f, py, px, p.height, p.width, spix);
          o.m[j][e] = (half_t)0.0f;
          o.v[j][e] = (half_t)0.0f;
          if (in) {
            const int my = nearest_src(py, p.sy, p.mask_h), mx = nearest_src(px, p.sx, p.mask_w);
            o.m[j][e] = masks[(mrow + my) * p.mask_w + mx];
            o.v[j][e] = src[spix];
          }
        }
      }
    }
  }
};

template <class L, Src S, bool SEL, int NOBJ>
__device__ __forceinline__ void blend_scatter(const PnpArgs& p, int nvar, unsigned active, const int* __restrict__ tab) {
  L it;
  if (!it.init(p)) return;
  half_t* x = p.x[blockIdx.y];
  Objs<S, NOBJ, L::W, L::NM> o;
  it.template load<S, NOBJ>(p, x, p.masks, tab, o);
  half_t t[L::W];
  if (p.base_chunk0) {  // one blend for every injecting variant
    ld_vec<L::W>(t, x + it.off);
    blend(t, o, t);
  }
  for (int k = 0; k < nvar; ++k) {
    if constexpr (SEL)
      if (!((active >> k) & 1u)) continue;
    half_t* cond = x + var_dst(p, nvar, p.ndst - 1, k) * it.chunk + it.off;
    if (!p.base_chunk0) {
      ld_vec<L::W>(t, cond);
      blend(t, o, t);
    }
    if (p.ndst == 2) st_vec<L::W>(x + var_dst(p, nvar, 0, k) * it.chunk + it.off, t);
    st_vec<L::W>(cond, t);
  }
}

// An offset table and masks PER VARIANT: place is [nvar][nobj][frames][2], masks are [nvar][nobj][frames][mask_h][mask_w]
// (variant k's masks in ITS destination coordinates).  The variant loop is the OUTER loop and only one variant's NOBJ object
// vectors are live at a time; next to them the kernels keep the base vector and the loop state, so they need more registers
// than the _placed kernels (DESIGN.md 6l has the table and what it costs).  With base_chunk0 the base vector is loaded once per
// work item and every injecting variant blends it with its own objects (the blend differs per variant, so it cannot be shared
// as in blend_scatter); otherwise variant k's base is its own cond chunk.
template <class L, int NOBJ>
__device__ __forceinline__ void blend_scatter_per_variant(const PnpArgs& p, int nvar, unsigned active, const int* __restrict__ place) {
  L it;
  if (!it.init(p)) return;
  half_t* x = p.x[blockIdx.y];
  const long mvar = (long)NOBJ * p.frames * p.mask_h * p.mask_w;  // masks of one variant
  half_t base[L::W];
  if (p.base_chunk0) ld_vec<L::W>(base, x + it.off);
  for (int k = 0; k < nvar; ++k) {
    if (!((active >> k) & 1u)) continue;
    Objs<SHIFT, NOBJ, L::W, L::NM> o;
    it.per_variant().template load<SHIFT, NOBJ>(p, x, p.masks + k * mvar, place + (long)k * NOBJ * p.frames * 2, o);
    half_t* cond = x + var_dst(p, nvar, p.ndst - 1, k) * it.chunk + it.off;
    if (!p.base_chunk0) ld_vec<L::W>(base, cond);
    half_t t[L::W];
    blend(base, o, t);
    if (p.ndst == 2) st_vec<L::W>(x + var_dst(p, nvar, 0, k) * it.chunk + it.off, t);
    st_vec<L::W>(cond, t);
  }
}

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
  blend_scatter_per_variant<Tokens, NOBJ>(p, nvar, active, place);
}

template <int VEC, int NOBJ>
__global__ __launch_bounds__(256) void pnp_nchw_placed_variants_kernel(const PnpArgs p, const int nvar, const unsigned active,
                                                                       const int* __restrict__ place) {
  blend_scatter_per_variant<Nchw<VEC>, NOBJ>(p, nvar, active, place);
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

int fill_args(const mvoc_pnp_desc* d, PnpArgs& a) {
  MVOC_REQUIRE(d && d->x && d->masks, -1, "pnp: null operand");
  MVOC_REQUIRE(d->nobj >= 1 && d->nobj <= 4, -2, "pnp: nobj %d not in [1,4]", d->nobj);
  MVOC_REQUIRE(d->frames > 0 && d->height > 0 && d->width > 0 && d->channels > 0 && d->mask_h > 0 && d->mask_w > 0, -1,
               "pnp: bad dims");
  a.x[0] = (half_t*)d->x;
  a.x[1] = (half_t*)d->x2;
  a.masks = (const half_t*)d->masks;
  a.chunk_stride = d->chunk_stride; a.f_stride = d->f_stride; a.p_stride = d->p_stride;
  a.nobj = d->nobj; a.frames = d->frames; a.height = d->height; a.width = d->width; a.channels = d->channels;
  a.mask_h = d->mask_h; a.mask_w = d->mask_w; a.base_chunk0 = d->base_chunk0;
  MVOC_REQUIRE(d->ndst >= 0 && d->ndst <= 2, -1, "pnp: ndst %d not in {0 (= 2), 1, 2}", d->ndst);
  a.ndst = d->ndst == 0 ? 2 : d->ndst;
  a.sy = (float)d->mask_h / (float)d->height;
  a.sx = (float)d->mask_w / (float)d->width;
  a.nsrc = d->nobj + 1;
  a.obj_map = 0;
  a.no_background = 0;
  return 0;
}

// base_chunk0 = -1 (no background chunk) is the positional tokens entry's alone: every other entry refuses it before it launches anything (a map
// expresses that layout already: nsrc = nobj, obj_chunk[j] = j; an _nchw entry blends features onto chunk 0, which is not there)
int refuse_no_background(const mvoc_pnp_desc* d, const char* entry) {
  MVOC_REQUIRE(!d || d->base_chunk0 != -1, -1,
               "%s: base_chunk0 = -1 (no background chunk) is taken by mvoc_pnp_blend_scatter_tokens only (a mapped entry expresses "
               "the layout as nsrc = nobj, obj_chunk[j] = j; the nchw entries need chunk 0)", entry);
  return 0;
}

// source map of the _mapped entries -> a.nsrc / a.obj_map; returns the number of DISTINCT source chunks the blend reads (the
// base included): repeated reads of one chunk hit the same lines back to back, so HBM serves each distinct chunk once
int fill_map(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk_host, PnpArgs& a, int& nread) {
  MVOC_REQUIRE(obj_chunk_host, -1, "pnp mapped: null obj_chunk");
  MVOC_REQUIRE(nsrc >= 1 && nsrc <= d->nobj + 1, -1, "pnp mapped: nsrc %d not in [1, nobj + 1 = %d]", nsrc, d->nobj + 1);
  unsigned map = 0, seen = d->base_chunk0 ? 1u : 0u;  // bit c: chunk c is read (the base when it is chunk 0)
  for (int j = 0; j < d->nobj; ++j) {
    const int c = obj_chunk_host[j];
    MVOC_REQUIRE(c >= 0 && c < nsrc, -1, "pnp mapped: obj_chunk[%d] = %d not in [0, nsrc = %d)", j, c, nsrc);
    map |= (unsigned)c << (4 * j);
    seen |= 1u << c;
  }
  a.nsrc = nsrc;
  a.obj_map = map;
  nread = __builtin_popcount(seen) + (d->base_chunk0 ? 0 : 1);  // + the last chunk as the base
  return 0;
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

// ---- host launch of the blend family ------------------------------------------------------------------------------------------
// What every entry of a layout derives from the descriptor: prepare_* checks the layout's preconditions, sets a.total and fills
// this; blend_bytes is the traffic the entry reports to the profiler; dispatch picks the instantiation.
struct Launch {
  dim3 grid;
  hipStream_t s;
  int ntens;
  bool vec;              // nchw: 8 pixels per work item (H * W a multiple of 8); tokens: always 8 channels
  double elems, pixels;  // F * H * W * C and F * H * W
};

int finish_prepare(const mvoc_pnp_desc* d, const PnpArgs& a, void* stream, Launch& l, const char* too_large) {
  const long nblk = (a.total + 255) / 256;
  MVOC_REQUIRE(nblk < 0x7fffffffL, -2, "%s", too_large);
  l.ntens = d->x2 ? 2 : 1;
  l.grid = dim3((unsigned)nblk, l.ntens);
  l.s = (hipStream_t)stream;
  l.pixels = (double)d->frames * d->height * d->width;
  l.elems = l.pixels * d->channels;
  return 0;
}

int prepare_tokens(const mvoc_pnp_desc* d, PnpArgs& a, void* stream, Launch& l) {
  MVOC_REQUIRE(d->channels % 8 == 0 && d->chunk_stride % 8 == 0 && d->f_stride % 8 == 0 && d->p_stride % 8 == 0, -2,
               "pnp tokens: channels/strides must be multiples of 8");
  l.vec = true;
  a.total = (long)d->frames * d->height * d->width * (d->channels / 8);
  return finish_prepare(d, a, stream, l, "pnp tokens: grid too large");
}

int prepare_nchw(const mvoc_pnp_desc* d, PnpArgs& a, void* stream, Launch& l) {
  const long hw = (long)d->height * d->width;
  l.vec = hw % 8 == 0;
  a.total = (long)d->frames * d->channels * (l.vec ? hw / 8 : hw);
  return finish_prepare(d, a, stream, l, "pnp nchw: grid too large");
}

// per tensor: `chunks` chunks of features read or written + `mask_sets` sets of nobj masks; + the bytes of a device table
double blend_bytes(const Launch& l, int nobj, double chunks, double mask_sets = 1.0, double table = 0.0) {
  return l.ntens * (l.elems * 2.0 * chunks + 2.0 * mask_sets * nobj * l.pixels) + table;
}

// f(NOBJ, VEC) as integral constants: nobj in [1, 4] (fill_args), VEC = 8 or 1 (the tokens kernels have no VEC and ignore it)
template <class F>
void dispatch(int nobj, bool vec, F&& f) {
  auto by_vec = [&](auto n) {
    if (vec) f(n, std::integral_constant<int, 8>{});
    else f(n, std::integral_constant<int, 1>{});
  };
  switch (nobj) {
    case 1: by_vec(std::integral_constant<int, 1>{}); break;
    case 2: by_vec(std::integral_constant<int, 2>{}); break;
    case 3: by_vec(std::integral_constant<int, 3>{}); break;
    default: by_vec(std::integral_constant<int, 4>{}); break;
  }
}

template <class K, class... Args>
void launch(K kernel, const Launch& l, Args... args) {
  hipLaunchKernelGGL(kernel, l.grid, dim3(256), 0, l.s, args...);
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

// _sel: distinct sources read (+ one base per INJECTING variant unless the base is chunk 0), ndst chunks written per injecting variant
int fill_variants_sel(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active, PnpArgs& a,
                      double& chunks) {
  MVOC_REQUIRE(nvar >= 1 && nvar <= 8, -1, "pnp variants: nvar %d not in [1, 8]", nvar);
  MVOC_REQUIRE(active != 0 && active < (1u << nvar), -1, "pnp variants: active mask 0x%x not in [1, 2^nvar = %u)", active,
               1u << nvar);
  int nread = 0;
  if (int rc = fill_args(d, a)) return rc;
  if (int rc = fill_map(d, nsrc, obj_chunk, a, nread)) return rc;
  const int on = __builtin_popcount(active);
  chunks = (d->base_chunk0 ? nread : nread - 1 + on) + (double)a.ndst * on;
  return 0;
}

// variants: every variant injects (an nvar outside [1, 8] is refused before the mask is looked at)
int fill_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, PnpArgs& a, double& chunks) {
  return fill_variants_sel(d, nsrc, obj_chunk, nvar, nvar >= 1 && nvar <= 8 ? (1u << nvar) - 1 : 0u, a, chunks);
}

// _placed: the _sel contract (nvar = 1 and every bit of `active` set are allowed) + the device table of feature offsets
int fill_placed(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active, const void* place,
                PnpArgs& a, double& chunks) {
  MVOC_REQUIRE(place, -1, "pnp placed: null offset table");
  return fill_variants_sel(d, nsrc, obj_chunk, nvar, active, a, chunks);
}

// _placed_variants: the _placed contract with a table and masks per variant.  Traffic in chunks: every injecting variant reads
// the distinct object chunks at its own pixels (nobjc each) and writes ndst chunks; the base is read once when it is chunk 0,
// else once per injecting variant
int fill_placed_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active,
                         const void* place, PnpArgs& a, double& chunks, int& on) {
  double unused = 0;
  if (int rc = fill_placed(d, nsrc, obj_chunk, nvar, active, place, a, unused)) return rc;
  unsigned seen = 0;
  for (int j = 0; j < d->nobj; ++j) seen |= 1u << obj_chunk[j];
  on = __builtin_popcount(active);
  chunks = (double)on * __builtin_popcount(seen) + (d->base_chunk0 ? 1 : on) + (double)a.ndst * on;
  return 0;
}

// _resampled: the _placed contract with the table of per-axis index maps in place of the offset table
int fill_resampled(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active, const void* maps,
                   PnpArgs& a, double& chunks) {
  MVOC_REQUIRE(maps, -1, "pnp resampled: null map table");
  return fill_variants_sel(d, nsrc, obj_chunk, nvar, active, a, chunks);
}

}  // namespace

extern "C" int mvoc_pnp_blend_scatter_tokens_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                      int32_t nvar, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_tokens_variants")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  if (int rc = fill_variants(d, nsrc, obj_chunk, nvar, a, chunks)) return rc;
  if (int rc = prepare_tokens(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks));
  dispatch(d->nobj, l.vec, [&](auto n, auto) { launch(pnp_tokens_variants_kernel<n.value>, l, a, (int)nvar); });
  return mvoc_check_launch("pnp_tokens_variants_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_nchw_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                    int32_t nvar, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_nchw_variants")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  if (int rc = fill_variants(d, nsrc, obj_chunk, nvar, a, chunks)) return rc;
  if (int rc = prepare_nchw(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks));
  dispatch(d->nobj, l.vec, [&](auto n, auto v) { launch(pnp_nchw_variants_kernel<v.value, n.value>, l, a, (int)nvar); });
  return mvoc_check_launch("pnp_nchw_variants_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_tokens_variants_sel(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                          int32_t nvar, uint32_t active, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_tokens_variants_sel")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  if (int rc = fill_variants_sel(d, nsrc, obj_chunk, nvar, active, a, chunks)) return rc;
  if (int rc = prepare_tokens(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks));
  dispatch(d->nobj, l.vec, [&](auto n, auto) { launch(pnp_tokens_variants_sel_kernel<n.value>, l, a, (int)nvar, (unsigned)active); });
  return mvoc_check_launch("pnp_tokens_variants_sel_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_nchw_variants_sel(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                        int32_t nvar, uint32_t active, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_nchw_variants_sel")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  if (int rc = fill_variants_sel(d, nsrc, obj_chunk, nvar, active, a, chunks)) return rc;
  if (int rc = prepare_nchw(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks));
  dispatch(d->nobj, l.vec,
           [&](auto n, auto v) { launch(pnp_nchw_variants_sel_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active); });
  return mvoc_check_launch("pnp_nchw_variants_sel_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_tokens_placed(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                    uint32_t active, const int32_t* place, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_tokens_placed")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  if (int rc = fill_placed(d, nsrc, obj_chunk, nvar, active, place, a, chunks)) return rc;
  if (int rc = prepare_tokens(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks));
  dispatch(d->nobj, l.vec, [&](auto n, auto) {
    launch(pnp_tokens_placed_kernel<n.value>, l, a, (int)nvar, (unsigned)active, (const int*)place);
  });
  return mvoc_check_launch("pnp_tokens_placed_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_nchw_placed(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                  uint32_t active, const int32_t* place, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_nchw_placed")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  if (int rc = fill_placed(d, nsrc, obj_chunk, nvar, active, place, a, chunks)) return rc;
  if (int rc = prepare_nchw(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks));
  dispatch(d->nobj, l.vec, [&](auto n, auto v) {
    launch(pnp_nchw_placed_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active, (const int*)place);
  });
  return mvoc_check_launch("pnp_nchw_placed_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_tokens_placed_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                             int32_t nvar, uint32_t active, const int32_t* place, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_tokens_placed_variants")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  int on = 0;
  if (int rc = fill_placed_variants(d, nsrc, obj_chunk, nvar, active, place, a, chunks, on)) return rc;
  if (int rc = prepare_tokens(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks, on, 8.0 * nvar * d->nobj * d->frames));
  dispatch(d->nobj, l.vec, [&](auto n, auto) {
    launch(pnp_tokens_placed_variants_kernel<n.value>, l, a, (int)nvar, (unsigned)active, (const int*)place);
  });
  return mvoc_check_launch("pnp_tokens_placed_variants_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_nchw_placed_variants(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk,
                                                           int32_t nvar, uint32_t active, const int32_t* place, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_nchw_placed_variants")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  int on = 0;
  if (int rc = fill_placed_variants(d, nsrc, obj_chunk, nvar, active, place, a, chunks, on)) return rc;
  if (int rc = prepare_nchw(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks, on, 8.0 * nvar * d->nobj * d->frames));
  dispatch(d->nobj, l.vec, [&](auto n, auto v) {
    launch(pnp_nchw_placed_variants_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active, (const int*)place);
  });
  return mvoc_check_launch("pnp_nchw_placed_variants_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_tokens_resampled(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                       uint32_t active, const int32_t* maps, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_tokens_resampled")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  if (int rc = fill_resampled(d, nsrc, obj_chunk, nvar, active, maps, a, chunks)) return rc;
  if (int rc = prepare_tokens(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s,
                     blend_bytes(l, d->nobj, chunks, 1.0, 4.0 * d->nobj * d->frames * ((double)d->height + d->width)));
  dispatch(d->nobj, l.vec, [&](auto n, auto) {
    launch(pnp_tokens_resampled_kernel<n.value>, l, a, (int)nvar, (unsigned)active, (const int*)maps);
  });
  return mvoc_check_launch("pnp_tokens_resampled_kernel");
}

extern "C" int mvoc_pnp_blend_scatter_nchw_resampled(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar,
                                                     uint32_t active, const int32_t* maps, void* stream) {
  if (int rc = refuse_no_background(d, "mvoc_pnp_blend_scatter_nchw_resampled")) return rc;
  PnpArgs a;
  Launch l;
  double chunks = 0;
  if (int rc = fill_resampled(d, nsrc, obj_chunk, nvar, active, maps, a, chunks)) return rc;
  if (int rc = prepare_nchw(d, a, stream, l)) return rc;
  MvocProfScope prof(MVOC_FAM_PNP, l.s,
                     blend_bytes(l, d->nobj, chunks, 1.0, 4.0 * d->nobj * d->frames * ((double)d->height + d->width)));
  dispatch(d->nobj, l.vec, [&](auto n, auto v) {
    launch(pnp_nchw_resampled_kernel<v.value, n.value>, l, a, (int)nvar, (unsigned)active, (const int*)maps);
  });
  return mvoc_check_launch("pnp_nchw_resampled_kernel");
}

extern "C" int mvoc_gather_planes_f16(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w,
                                      const int32_t* maps, void* stream) {
  MVOC_REQUIRE(src && dst && maps, -1, "gather_planes: null operand");
  MVOC_REQUIRE(src != dst, -1, "gather_planes: in place (src == dst) is not supported");
  MVOC_REQUIRE(nplane > 0 && frames > 0 && h > 0 && w > 0, -1, "gather_planes: bad dims");
  const long n = (long)nplane * frames * h * w;
  const long nblk = (n + 255) / 256;
  MVOC_REQUIRE(nblk < 0x7fffffffL, -2, "gather_planes: grid too large");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * n * 2 + 4.0 * frames * ((double)h + w));
  hipLaunchKernelGGL(gather_planes_kernel, dim3((unsigned)nblk), dim3(256), 0, s, (const half_t*)src, (half_t*)dst, (int)frames,
                     (int)h, (int)w, (const int*)maps, n);
  return mvoc_check_launch("gather_planes_kernel");
}

extern "C" int mvoc_shift_planes_f16(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w,
                                     const int32_t* offsets, void* stream) {
  MVOC_REQUIRE(src && dst && offsets, -1, "shift_planes: null operand");
  MVOC_REQUIRE(src != dst, -1, "shift_planes: in place (src == dst) is not supported");
  MVOC_REQUIRE(nplane > 0 && frames > 0 && h > 0 && w > 0, -1, "shift_planes: bad dims");
  const long n = (long)nplane * frames * h * w;
  const long nblk = (n + 255) / 256;
  MVOC_REQUIRE(nblk < 0x7fffffffL, -2, "shift_planes: grid too large");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * n * 2);
  hipLaunchKernelGGL(shift_planes_kernel, dim3((unsigned)nblk), dim3(256), 0, s, (const half_t*)src, (half_t*)dst, (int)frames,
                     (int)h, (int)w, (const int*)offsets, n);
  return mvoc_check_launch("shift_planes_kernel");
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
