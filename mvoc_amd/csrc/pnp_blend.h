// The pieces of the blend-scatter family that more than one translation unit composes its kernels
// from: the argument block and what fills / refuses it, the fp16 blend, the two item geometries with their object loads, the
// per-variant scatter and the host path: the table forms (one row each), run_entry (the one body of every entry that takes
// variants), move_planes (the one body of the plane movers) and what they launch through.  pnp.hip holds the
// family's ten kernels (and the text that describes the pieces), the two nearest plane movers and their entries;
// pnp_variants2.hip the per-variant MAP form; pnp_warp.hip the MAP2 form (a 2-D index map: rotation);
// pnp_bilinear.hip the TAPS form (four taps and fixed-point weights per pixel: bilinear sampling) -- each unit its
// kernels and one call per entry.  Everything is in an anonymous namespace: each unit gets its own copy.
#pragma once
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

// MAP2: map = int32 [nobj][frames][height * width], the linear source pixel sy * width + sx of every destination pixel -- a device
// table for THIS site's H x W, constant for the whole call (a rotation is not separable into per-axis maps).  One
// UNSIGNED compare against height * width takes the negative and the too-large entries alike: every int32 entry is safe.
__device__ __forceinline__ bool warped_src(const int* __restrict__ map, int j, int frames, int f, int py, int px, int h, int w,
                                           long& spix) {
  const unsigned s = (unsigned)map[((long)j * frames + f) * h * w + py * w + px];
  spix = (long)s;
  return s < (unsigned)(h * w);
}

enum Src { DIRECT, SHIFT, MAP, MAP2, TAPS };

// TAPS: taps = int32 [nobj][frames][height * width][2], bilinear sampling on an exact fp16 chain.  Word 0 =
// ((y0 + 1) << 16) | (x0 + 1) names the upper-left tap (y0 in [-1, h - 1], x0 in [-1, w - 1]; -1 by convention where the object is
// absent), word 1 = (qy << 16) | qx the weights of the LOWER row and the RIGHT column in 1/256 (9 bits each are read).  A tap's
// VALUE is used only if (unsigned)row < h && (unsigned)col < w; a tap outside still issues a load, of the plane's pixel 0 (always in
// bounds), and the loaded bits are ANDed to +0.0 before they enter the chain -- so every int32 pair is safe and no load is behind
// a branch.  The object is present iff at least one tap is inside the plane.  lerp16_h is blend16_h with free weights: one correctly rounded fp16 operation per statement.
__device__ __forceinline__ half_t lerp16_h(half_t a, half_t b, half_t w0, half_t w1) {
  const half_t x = a * w0;
  const half_t y = b * w1;
  return x + y;
}

struct Taps {
  int s[4];       // source pixels of the taps (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1); 0 where the tap is outside
  unsigned bits;  // bit k: tap k is inside the plane; bit 4: any of them is (the object is present)
  half_t wx0, wx1, wy0, wy1;
};

// The flags travel as ONE opaque VGPR per (object, pixel) and each becomes an all-ones / zero AND mask where it is used: as bools
// they are wave-wide conditions in SGPR pairs that stay live across the loads, and the 8-pixel NCHW forms spill SGPRs.  A value
// whose tap is outside is ANDed to +0.0.
__device__ __forceinline__ unsigned short tap_mask(unsigned bits, int k) {
  return (unsigned short)(-(int)((bits >> k) & 1u));
}

__device__ __forceinline__ half_t tap_and(half_t v, unsigned short m) {
  unsigned short u;
  __builtin_memcpy(&u, &v, 2);
  u &= m;
  __builtin_memcpy(&v, &u, 2);
  return v;
}

__device__ __forceinline__ Taps taps_src(const int* __restrict__ taps, int j, int frames, int f, int py, int px, int h, int w) {
  const int2 t = *reinterpret_cast<const int2*>(taps + ((((long)j * frames + f) * h + py) * w + px) * 2);
  const unsigned r0 = ((unsigned)t.x >> 16) - 1u, c0 = ((unsigned)t.x & 0xffffu) - 1u;
  const unsigned r1 = r0 + 1u, c1 = c0 + 1u;
  const bool ri0 = r0 < (unsigned)h, ri1 = r1 < (unsigned)h, ci0 = c0 < (unsigned)w, ci1 = c1 < (unsigned)w;
  Taps o;
  o.s[0] = ri0 && ci0 ? (int)(r0 * w + c0) : 0;
  o.s[1] = ri0 && ci1 ? (int)(r0 * w + c1) : 0;
  o.s[2] = ri1 && ci0 ? (int)(r1 * w + c0) : 0;
  o.s[3] = ri1 && ci1 ? (int)(r1 * w + c1) : 0;
  o.bits = (ri0 && ci0 ? 1u : 0u) | (ri0 && ci1 ? 2u : 0u) | (ri1 && ci0 ? 4u : 0u) | (ri1 && ci1 ? 8u : 0u) |
           ((ri0 || ri1) && (ci0 || ci1) ? 16u : 0u);
  asm volatile("" : "+v"(o.bits));
  const int qy = (t.y >> 16) & 0x1ff, qx = t.y & 0x1ff;
  const half_t u = (half_t)0.00390625f;  // 1/256: the products are exact for q <= 256
  o.wx0 = (half_t)(256 - qx) * u, o.wx1 = (half_t)qx * u;
  o.wy0 = (half_t)(256 - qy) * u, o.wy1 = (half_t)qy * u;
  return o;
}

// the four loaded values -> the interpolated value (0 where the object is absent)
__device__ __forceinline__ half_t taps_value(const Taps& t, half_t v00, half_t v01, half_t v10, half_t v11) {
  v00 = tap_and(v00, tap_mask(t.bits, 0)), v01 = tap_and(v01, tap_mask(t.bits, 1));
  v10 = tap_and(v10, tap_mask(t.bits, 2)), v11 = tap_and(v11, tap_mask(t.bits, 3));
  const half_t top = lerp16_h(v00, v01, t.wx0, t.wx1);
  const half_t bot = lerp16_h(v10, v11, t.wx0, t.wx1);
  return tap_and(lerp16_h(top, bot, t.wy0, t.wy1), tap_mask(t.bits, 4));
}

template <Src S>
__device__ __forceinline__ bool obj_src(const int* __restrict__ tab, int j, int frames, int f, int py, int px, int h, int w,
                                        long& spix) {
  if constexpr (S == SHIFT) return placed_src(tab, j, frames, f, py, px, h, w, spix);
  else if constexpr (S == MAP) return resampled_src(tab, j, frames, f, py, px, h, w, spix);
  else return warped_src(tab, j, frames, f, py, px, h, w, spix);
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

  // (see Nchw::per_variant) SHIFT: nothing to do, the hoisted terms are few.  MAP: the eight table-row and four mask indices of
  // NOBJ = 4 are 64-bit and loop-invariant; hoisted they cost the form its eighth wave (67 VGPRs).  An opaque frame index forms
  // them inside the loop.
  template <Src S>
  __device__ __forceinline__ Tokens per_variant() const {
    Tokens it = *this;
    if constexpr (S == MAP) asm volatile("" : "+v"(it.f));
    return it;
  }

  template <Src S, int NOBJ>
  __device__ __forceinline__ void load(const PnpArgs& p, const half_t* x, const half_t* masks, const int* __restrict__ tab,
                                       Objs<S, NOBJ, 8, 1>& o) const {
#pragma unroll
    for (int j = 0; j < NOBJ; ++j) {
      const half_t* src = x + obj_chunk<true>(p, j) * chunk;
      if constexpr (S == DIRECT) {
        o.m[j][0] = (float)masks[mask_index(p, j, f, my, mx)];
        ld_vec<8>(o.v[j], src + off);
      } else if constexpr (S == TAPS) {
        // the four vectors are loaded without a branch (a tap outside reads pixel 0 and is ANDed to +0.0): all four loads are in
        // flight before the first is consumed
        const Taps t = taps_src(tab, j, p.frames, f, py, px, p.height, p.width);
        half_t v[4][8];
#pragma unroll
        for (int k = 0; k < 4; ++k) ld_vec<8>(v[k], src + foff + (long)t.s[k] * p.p_stride);
        o.m[j][0] = tap_and(masks[mask_index(p, j, f, my, mx)], tap_mask(t.bits, 4));
#pragma unroll
        for (int e = 0; e < 8; ++e) o.v[j][e] = taps_value(t, v[0][e], v[1][e], v[2][e], v[3][e]);
        // 3 and 4 objects: an opaque use of the finished vector, so that this object's interpolation ends before the next
        // object's loads are issued -- with all sixteen tap vectors in flight the kernel needs 74 / 108 VGPRs (6 / 4 waves), this
        // way 57 (8 waves)
        if constexpr (NOBJ > 2) asm volatile("" : "+v"(*reinterpret_cast<half8_t*>(o.v[j])));
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
  template <Src S>
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
          if constexpr (S == TAPS) {
            const Taps t = taps_src(tab, j, p.frames, f, py, px, p.height, p.width);
            half_t v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = src[t.s[k]];
            const int my = nearest_src(py, p.sy, p.mask_h), mx = nearest_src(px, p.sx, p.mask_w);
            o.m[j][e] = tap_and(masks[(mrow + my) * p.mask_w + mx], tap_mask(t.bits, 4));
            o.v[j][e] = taps_value(t, v[0], v[1], v[2], v[3]);
          } else {
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
  }
};

// The variant scatter with the objects loaded ONCE (pnp.hip has the text on the pieces and the kernels made of them)
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

// A table and masks PER VARIANT: masks are [nvar][nobj][frames][mask_h][mask_w] (variant k's masks in ITS destination
// coordinates), the table is [nvar][nobj][frames][2] (S = SHIFT: offsets) or [nvar][nobj][frames][height + width]
// (S = MAP: per-axis index maps); variant k's rows start at k * NOBJ * frames * 2 or k * NOBJ * frames * (height +
// width), formed in 64 bits.  The variant loop is the OUTER loop and only one variant's NOBJ object vectors are live at a time;
// next to them the kernels keep the base vector and the loop state, so they need more registers than the shared-table kernels
// (DESIGN.md 6l and 6o have the tables and what it costs).  With base_chunk0 the base vector is loaded once per work item and
// every injecting variant blends it with its own objects (the blend differs per variant, so it cannot be shared as in
// blend_scatter); otherwise variant k's base is its own cond chunk.
template <class L, Src S, int NOBJ>
__device__ __forceinline__ void blend_scatter_per_variant(const PnpArgs& p, int nvar, unsigned active, const int* __restrict__ tab) {
  static_assert(S != DIRECT, "a per-variant blend reads its objects through a table");
  L it;
  if (!it.init(p)) return;
  half_t* x = p.x[blockIdx.y];
  const long mvar = (long)NOBJ * p.frames * p.mask_h * p.mask_w;  // masks of one variant
  half_t base[L::W];
  if (p.base_chunk0) ld_vec<L::W>(base, x + it.off);
  for (int k = 0; k < nvar; ++k) {
    if (!((active >> k) & 1u)) continue;
    Objs<S, NOBJ, L::W, L::NM> o;
    const int* vtab;
    if constexpr (S == SHIFT) vtab = tab + (long)k * NOBJ * p.frames * 2;
    else vtab = tab + (long)k * NOBJ * p.frames * ((long)p.height + p.width);
    it.template per_variant<S>().template load<S, NOBJ>(p, x, p.masks + k * mvar, vtab, o);
    half_t* cond = x + var_dst(p, nvar, p.ndst - 1, k) * it.chunk + it.off;
    if (!p.base_chunk0) ld_vec<L::W>(base, cond);
    half_t t[L::W];
    blend(base, o, t);
    if (p.ndst == 2) st_vec<L::W>(x + var_dst(p, nvar, 0, k) * it.chunk + it.off, t);
    st_vec<L::W>(cond, t);
  }
}

// ---- host: filling and refusing the argument block ----------------------------------------------------------------------------
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

// `active` of the entries without one: every variant injects (an nvar outside [1, 8] is refused before the mask is looked at)
uint32_t all_variants(int32_t nvar) { return nvar >= 1 && nvar <= 8 ? (1u << nvar) - 1 : 0u; }

// ---- host: the table forms ----------------------------------------------------------------------------------------------------
// A table form is what an entry adds to the _sel contract (nvar = 1 and every bit of `active` set are allowed) when its kernels
// read the objects through a device table: the source rule S of the object load, whether there is a table and a mask set per
// variant, and what the host refuses for it.  One row per form; run_entry and move_planes read nothing else, so a new form is a
// row here, its object load above and its kernels and entries in a unit.
struct TableForm {
  Src src;                 // the table's row per (object, frame): table_words
  bool per_variant;        // [nvar][nobj][frames][..] with masks [nvar][nobj][frames][mask_h][mask_w]
  const char* null_table;  // the refusal of a null table; nullptr: the entry takes none
  const char* blend;       // who speaks when a blend entry misses the form's limits
  const char* mover;       // the form's plane mover, as it names itself in every refusal
  const char* hw_fits;     // MAP2 / TAPS: the kernels form height * width as an int and (MAP2) a map entry is an int32 -- what a
                           // site of 2^31 pixels or more does not fit; nullptr: no such limit
};

constexpr TableForm NO_TABLE = {DIRECT, false, nullptr, nullptr, nullptr, nullptr};
constexpr TableForm PLACED = {SHIFT, false, "pnp placed: null offset table", nullptr, "shift_planes", nullptr};
constexpr TableForm PLACED_VARIANTS = {SHIFT, true, "pnp placed: null offset table", nullptr, nullptr, nullptr};
constexpr TableForm RESAMPLED = {MAP, false, "pnp resampled: null map table", nullptr, "gather_planes", nullptr};
constexpr TableForm RESAMPLED_VARIANTS = {MAP, true, "pnp resampled variants: null map table", nullptr, nullptr, nullptr};
constexpr TableForm WARPED = {MAP2, false, "pnp warped: null map table", "pnp warped", "gather_planes_warped", "the int32 map entries"};
constexpr TableForm BILINEAR = {TAPS, false, "pnp bilinear: null tap table", "pnp bilinear", "gather_planes_bilinear", "an int"};

// int32 words of one table row: [2], [h + w], [h * w] or [h * w][2]
double table_words(Src s, double h, double w) {
  switch (s) {
    case SHIFT: return 2.0;
    case MAP: return h + w;
    case MAP2: return h * w;
    case TAPS: return 2.0 * h * w;
    default: return 0.0;
  }
}

// the table's bytes as the profiler is told them, `rows` = (variants x) objects x frames rows.  The offset table shared by the
// variants (8 bytes per row) has never been counted, by the _placed entries or by shift_planes
double table_bytes(const TableForm& t, double rows, int h, int w) {
  if (t.src == SHIFT && !t.per_variant) return 0.0;
  return 4.0 * rows * table_words(t.src, h, w);
}

// the form's limits on a site of h x w; `hname` / `wname`: what the caller's interface calls them.  TAPS: a tap row / column + 1
// is a 16-bit field of word 0 and 0xffff is kept for "absent": a site with 65 535 rows or columns or more is refused
int table_limits(const TableForm& t, const char* who, const char* hname, const char* wname, int h, int w) {
  MVOC_REQUIRE(!t.hw_fits || (long)h * w < 0x7fffffffL, -2, "%s: %s * %s does not fit %s", who, hname, wname, t.hw_fits);
  MVOC_REQUIRE(t.src != TAPS || (h < 65535 && w < 65535), -2, "%s: %s %d or %s %d does not fit the 16-bit tap fields (< 65535)", who,
               hname, h, wname, w);
  return 0;
}

// ---- host launch of the blend family ------------------------------------------------------------------------------------------
// What every entry of a layout derives from the descriptor: prepare_* checks the layout's preconditions, sets a.total and fills
// this; blend_bytes is the traffic the entry reports to the profiler; dispatch picks the instantiation.
struct Launch {
  dim3 grid;
  hipStream_t s;
  int ntens;
  bool vec;              // nchw: 8 pixels per work item (H * W a multiple of 8, x / x2 16-byte aligned); tokens: always 8 channels
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
  // every access of the tokens kernels is a 16-byte vector at x + a multiple of 8 elements
  MVOC_REQUIRE(((uintptr_t)d->x | (uintptr_t)d->x2) % 16 == 0, -2, "pnp tokens: x and x2 must be 16-byte aligned");
  l.vec = true;
  a.total = (long)d->frames * d->height * d->width * (d->channels / 8);
  return finish_prepare(d, a, stream, l, "pnp tokens: grid too large");
}

int prepare_nchw(const mvoc_pnp_desc* d, PnpArgs& a, void* stream, Launch& l) {
  const long hw = (long)d->height * d->width;
  // the 8-wide form reads and writes 16-byte vectors at x + a multiple of 8 elements: it needs the pointers aligned as well
  l.vec = hw % 8 == 0 && ((uintptr_t)d->x | (uintptr_t)d->x2) % 16 == 0;
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

// What every entry that takes variants does, in the order its refusals are promised: no-background, null table, nvar, active, the
// descriptor, the source map, the form's limits, the layout's preconditions (`prepare` = prepare_tokens / prepare_nchw); then the
// profiler scope and `launch_inst(NOBJ, VEC, l, a)`, which launches the entry's kernel `kernel` in that instantiation.
template <class F>
int run_entry(const char* entry, const char* kernel, const TableForm& t, int (*prepare)(const mvoc_pnp_desc*, PnpArgs&, void*, Launch&),
              const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active, const void* table,
              void* stream, F&& launch_inst) {
  if (int rc = refuse_no_background(d, entry)) return rc;
  MVOC_REQUIRE(!t.null_table || table, -1, "%s", t.null_table);
  PnpArgs a;
  Launch l;
  double chunks = 0, mask_sets = 1.0;
  if (int rc = fill_variants_sel(d, nsrc, obj_chunk, nvar, active, a, chunks)) return rc;
  if (t.per_variant) {
    // a table and masks per variant.  Traffic in chunks: every injecting variant reads the distinct object chunks at its own
    // pixels and writes ndst chunks; the base is read once when it is chunk 0, else once per injecting variant
    unsigned seen = 0;
    for (int j = 0; j < d->nobj; ++j) seen |= 1u << obj_chunk[j];
    const int on = __builtin_popcount(active);
    chunks = (double)on * __builtin_popcount(seen) + (d->base_chunk0 ? 1 : on) + (double)a.ndst * on;
    mask_sets = on;
  }
  if (int rc = table_limits(t, t.blend, "height", "width", d->height, d->width)) return rc;
  if (int rc = prepare(d, a, stream, l)) return rc;
  const double rows = (t.per_variant ? (double)nvar : 1.0) * d->nobj * d->frames;
  MvocProfScope prof(MVOC_FAM_PNP, l.s, blend_bytes(l, d->nobj, chunks, mask_sets, table_bytes(t, rows, d->height, d->width)));
  dispatch(d->nobj, l.vec, [&](auto n, auto v) { launch_inst(n, v, l, a); });
  return mvoc_check_launch(kernel);
}

// What every plane mover does: [nplane][frames][h][w] fp16 planes through one table row per frame, shared by the planes.
// `launch_k(grid, stream, n)` launches the mover's kernel `kernel` over the n elements.
template <class F>
int move_planes(const TableForm& t, const char* kernel, const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h,
                int32_t w, const void* table, void* stream, F&& launch_k) {
  MVOC_REQUIRE(src && dst && table, -1, "%s: null operand", t.mover);
  MVOC_REQUIRE(src != dst, -1, "%s: in place (src == dst) is not supported", t.mover);
  MVOC_REQUIRE(nplane > 0 && frames > 0 && h > 0 && w > 0, -1, "%s: bad dims", t.mover);
  if (int rc = table_limits(t, t.mover, "h", "w", h, w)) return rc;
  const long n = (long)nplane * frames * h * w;
  const long nblk = (n + 255) / 256;
  MVOC_REQUIRE(nblk < 0x7fffffffL, -2, "%s: grid too large", t.mover);
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * n * 2 + table_bytes(t, frames, h, w));
  launch_k(dim3((unsigned)nblk), s, n);
  return mvoc_check_launch(kernel);
}

}  // namespace
