// Stem / small ops of the UNet (pipeline_i2vgen_xl.py:166-290, 351-357): a few MB of traffic per step,
// latency-bound.  Simple one-thread-per-output kernels on channels-last data.
#include "common.h"

namespace {

__global__ void timestep_embedding_kernel(const float* __restrict__ t, int nb, int dim, half_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = dim / 2;
  if (i >= nb * dim) return;
  const int b = i / dim, j = i % dim;
  const int k = j < half ? j : j - half;
  const float freq = expf(-logf(10000.0f) * (float)k / (float)half);
  const float ang = t[b] * freq;
  out[i] = (half_t)(j < half ? cosf(ang) : sinf(ang));
}

__global__ void act_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, long n, int act) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = (float)x[i];
  out[i] = (half_t)(act == MVOC_ACT_SILU ? silu_f(v) : act == MVOC_ACT_GELU ? gelu_erf_f(v) : v);
}

__global__ void add_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b, half_t* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = (half_t)((float)a[i] + (float)b[i]);
}

// x [nimg][h][w][cin] -> out [nimg][ho][wo][cout], 3x3, pad 1; thread = (pixel, cout)
__global__ void conv3x3_small_kernel(const half_t* __restrict__ x, const half_t* __restrict__ w,
                                     const half_t* __restrict__ bias, half_t* __restrict__ out, int nimg, int h, int wd,
                                     int cin, int cout, int stride, int ho, int wo, int silu) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)nimg * ho * wo * cout;
  if (i >= total) return;
  const int co = (int)(i % cout);
  long pix = i / cout;
  const int ox = (int)(pix % wo);
  pix /= wo;
  const int oy = (int)(pix % ho);
  const int img = (int)(pix / ho);
  float acc = 0.f;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * stride + ky - 1;
    if (iy < 0 || iy >= h) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox * stride + kx - 1;
      if (ix < 0 || ix >= wd) continue;
      const half_t* xp = x + (((long)img * h + iy) * wd + ix) * cin;
      const half_t* wp = w + ((long)co * 9 + ky * 3 + kx) * cin;
      for (int c = 0; c < cin; ++c) acc += (float)xp[c] * (float)wp[c];
    }
  }
  float v = r16(acc + (bias ? (float)bias[co] : 0.f));
  if (silu) v = silu_f(v);
  out[i] = (half_t)v;
}

__global__ void avgpool_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, int nimg, int h, int w, int c,
                               int oh, int ow) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)nimg * oh * ow * c;
  if (i >= total) return;
  const int ch = (int)(i % c);
  long pix = i / c;
  const int ox = (int)(pix % ow);
  pix /= ow;
  const int oy = (int)(pix % oh);
  const int img = (int)(pix / oh);
  const int y0 = (oy * h) / oh, y1 = ((oy + 1) * h + oh - 1) / oh;
  const int x0 = (ox * w) / ow, x1 = ((ox + 1) * w + ow - 1) / ow;
  float s = 0.f;
  for (int y = y0; y < y1; ++y)
    for (int xx = x0; xx < x1; ++xx) s += (float)x[(((long)img * h + y) * w + xx) * c + ch];
  out[i] = (half_t)(s / (float)((y1 - y0) * (x1 - x0)));
}

__global__ void ncfhw_to_tokens_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, int b, int c, int f, int hw,
                                       int ldo, int coff) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)b * f * hw;
  if (i >= total) return;
  const int p = (int)(i % hw);
  const long bf = i / hw;
  const int fi = (int)(bf % f), bi = (int)(bf / f);
  for (int ch = 0; ch < c; ++ch) out[i * ldo + coff + ch] = x[(((long)bi * c + ch) * f + fi) * hw + p];
}

__global__ void tokens_to_ncfhw_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, int b, int c, int f, int hw,
                                       int ld) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)b * c * f * hw;
  if (i >= total) return;
  const int p = (int)(i % hw);
  long r = i / hw;
  const int fi = (int)(r % f);
  r /= f;
  const int ch = (int)(r % c);
  const int bi = (int)(r / c);
  out[i] = x[(((long)bi * f + fi) * hw + p) * ld + ch];
}

// I2VGenXLTransformerTemporalEncoder, dim 4, 2 heads of 4, FF 4->16->4 (gelu).  thread = (sample, pixel, frame i)
struct Enc4Params {
  half_t ln_g[4], ln_b[4], wq[32], wk[32], wv[32], wo[32], bo[4], w1[64], b1[16], w2[64], b2[4];
};

__device__ __forceinline__ void enc4_ln(const half_t* xp, const Enc4Params& P, float* y) {
  float v[4], mean = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) { v[c] = (float)xp[c]; mean += v[c]; }
  mean *= 0.25f;
  float var = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) var += (v[c] - mean) * (v[c] - mean);
  const float rstd = rsqrtf(var * 0.25f + 1e-5f);
#pragma unroll
  for (int c = 0; c < 4; ++c) y[c] = r16((v[c] - mean) * rstd * (float)P.ln_g[c] + (float)P.ln_b[c]);
}

__global__ void temporal_encoder4_kernel(const half_t* __restrict__ x, const Enc4Params* __restrict__ params,
                                         half_t* __restrict__ out, int b, int f, int hw, int ldo, int coff) {
  __shared__ Enc4Params P;
  for (int i = threadIdx.x; i < (int)(sizeof(Enc4Params) / sizeof(half_t)); i += blockDim.x)
    reinterpret_cast<half_t*>(&P)[i] = reinterpret_cast<const half_t*>(params)[i];
  __syncthreads();
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)b * f * hw;
  if (idx >= total) return;
  const int p = (int)(idx % hw);
  const long bf = idx / hw;
  const int bi = (int)(bf / f);
  const half_t* xi = x + idx * 4;
  float yi[4], q[8];
  enc4_ln(xi, P, yi);
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) s += yi[c] * (float)P.wq[o * 4 + c];
    q[o] = r16(s);
  }
  // online softmax over the frames of this pixel, both heads
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f}, acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < f; ++j) {
    const half_t* xj = x + (((long)bi * f + j) * hw + p) * 4;
    float yj[4], k[8], v[8];
    enc4_ln(xj, P, yj);
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      float sk = 0.f, sv = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        sk += yj[c] * (float)P.wk[o * 4 + c];
        sv += yj[c] * (float)P.wv[o * 4 + c];
      }
      k[o] = r16(sk);
      v[o] = r16(sv);
    }
#pragma unroll
    for (int hd = 0; hd < 2; ++hd) {
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < 4; ++d) s += q[hd * 4 + d] * k[hd * 4 + d];
      s *= 0.5f;  // 1/sqrt(head_dim 4)
      const float mn = fmaxf(m[hd], s);
      const float a = __expf(m[hd] - mn), pj = __expf(s - mn);
      l[hd] = l[hd] * a + pj;
#pragma unroll
      for (int d = 0; d < 4; ++d) acc[hd * 4 + d] = acc[hd * 4 + d] * a + pj * v[hd * 4 + d];
      m[hd] = mn;
    }
  }
  float att[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) att[o] = r16(acc[o] / l[o >> 2]);
  float h1[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float s = 0.f;
#pragma unroll
    for (int o = 0; o < 8; ++o) s += att[o] * (float)P.wo[c * 8 + o];
    h1[c] = r16(r16(s + (float)P.bo[c]) + (float)xi[c]);
  }
  float ff[16];
#pragma unroll
  for (int o = 0; o < 16; ++o) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) s += h1[c] * (float)P.w1[o * 4 + c];
    ff[o] = r16(gelu_erf_f(r16(s + (float)P.b1[o])));
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float s = 0.f;
#pragma unroll
    for (int o = 0; o < 16; ++o) s += ff[o] * (float)P.w2[c * 16 + o];
    out[idx * ldo + coff + c] = (half_t)(r16(s + (float)P.b2[c]) + h1[c]);
  }
}

// busy-wait for `us` microseconds (s_memrealtime ticks at 100 MHz): lets the host run ahead of the GPU so that
// per-launch HIP-event brackets measure kernels, not launch gaps
__global__ void delay_kernel(long ticks) {
  const long t0 = __builtin_amdgcn_s_memrealtime();
  while ((long)__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

inline unsigned nblk(long n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }

// CLIP towers (clip.py): the two embedding stages either side of the transformer stacks
// non-overlapping patches of NCHW pixels -> im2col rows [B * g * g, kpad], k = (c, py, px) as Conv2d's weight.view(N, -1); pad = 0
__global__ __launch_bounds__(256) void clip_patches_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, int size, int patch,
                                                           int kpad, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int g = size / patch;
  const int k = (int)(i % kpad);
  const long row = i / kpad;
  half_t v = (half_t)0.f;
  if (k < 3 * patch * patch) {
    const int c = k / (patch * patch), py = (k / patch) % patch, px = k % patch;
    const int gx = (int)(row % g), gy = (int)((row / g) % g);
    const long b = row / ((long)g * g);
    v = x[((b * 3 + c) * size + gy * patch + py) * (long)size + gx * patch + px];
  }
  out[i] = v;
}

// out[row] = src(row) + pos[row % T]; src = table[ids[row]] (text tower) or, ids == NULL, the class embedding at t == 0 and
// patch row (row / T) * (T - 1) + t - 1 otherwise (vision tower)
__global__ __launch_bounds__(256) void clip_embed_kernel(const half_t* __restrict__ table, const int* __restrict__ ids,
                                                         const half_t* __restrict__ cls, const half_t* __restrict__ pos,
                                                         half_t* __restrict__ out, int T, int c8n, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c8 = (int)(i % c8n);
  const long row = i / c8n;
  const int t = (int)(row % T);
  const half_t* src;
  if (ids) src = table + ((long)ids[row] * c8n + c8) * 8;
  else if (t == 0) src = cls + c8 * 8;
  else src = table + (((row / T) * (T - 1) + t - 1) * c8n + c8) * 8;
  const half8_t a = *reinterpret_cast<const half8_t*>(src);
  const half8_t b = *reinterpret_cast<const half8_t*>(pos + ((long)t * c8n + c8) * 8);
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)a[e] + (float)b[e]);
  reinterpret_cast<half8_t*>(out)[i] = o;
}

}  // namespace

extern "C" int mvoc_timestep_embedding_f16(const float* t_dev, int32_t nb, int32_t dim, void* out, void* stream) {
  MVOC_REQUIRE(t_dev && out && nb > 0 && dim > 0 && dim % 2 == 0, -1, "timestep_embedding: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * nb * dim);
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3(nblk((long)nb * dim)), dim3(256), 0, s, t_dev, nb, dim, (half_t*)out);
  return mvoc_check_launch("timestep_embedding_kernel");
}

extern "C" int mvoc_act_f16(const void* x, void* out, int64_t n, int32_t act, void* stream) {
  MVOC_REQUIRE(x && out && n > 0, -1, "act: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 4.0 * n);
  hipLaunchKernelGGL(act_kernel, dim3(nblk(n)), dim3(256), 0, s, (const half_t*)x, (half_t*)out, (long)n, act);
  return mvoc_check_launch("act_kernel");
}

extern "C" int mvoc_add_f16(const void* a, const void* b, void* out, int64_t n, void* stream) {
  MVOC_REQUIRE(a && b && out && n > 0, -1, "add: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 6.0 * n);
  hipLaunchKernelGGL(add_kernel, dim3(nblk(n)), dim3(256), 0, s, (const half_t*)a, (const half_t*)b, (half_t*)out, (long)n);
  return mvoc_check_launch("add_kernel");
}

extern "C" int mvoc_conv3x3_small_f16(const void* x, const void* w, const void* bias, void* out, int32_t nimg, int32_t h,
                                      int32_t wd, int32_t cin, int32_t cout, int32_t stride, int32_t silu, void* stream) {
  MVOC_REQUIRE(x && w && out && nimg > 0 && h > 0 && wd > 0 && cin > 0 && cout > 0 && (stride == 1 || stride == 2), -1,
               "conv3x3_small: bad args");
  const int ho = (h + 2 - 3) / stride + 1, wo = (wd + 2 - 3) / stride + 1;
  const long total = (long)nimg * ho * wo * cout;
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * ((double)nimg * h * wd * cin + total));
  hipLaunchKernelGGL(conv3x3_small_kernel, dim3(nblk(total)), dim3(256), 0, s, (const half_t*)x, (const half_t*)w,
                     (const half_t*)bias, (half_t*)out, nimg, h, wd, cin, cout, stride, ho, wo, silu);
  return mvoc_check_launch("conv3x3_small_kernel");
}

// ---- VAE helpers -------------------------------------------------------------------------------------
// 1x1 conv over a handful of channels (AutoencoderKL.quant_conv 8 -> 8, post_quant_conv 4 -> 4): thread = (row, cout)
__global__ void conv1x1_small_kernel(const half_t* __restrict__ x, const half_t* __restrict__ w, const half_t* __restrict__ bias,
                                     half_t* __restrict__ out, long rows, int cin, int cout) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cout) return;
  const int co = (int)(i % cout);
  const long r = i / cout;
  float acc = 0.f;
  for (int c = 0; c < cin; ++c) acc += (float)x[r * cin + c] * (float)w[co * cin + c];
  out[i] = (half_t)(acc + (bias ? (float)bias[co] : 0.f));
}

// [n][c][hw] fp16 (reference NCHW images / latents) <-> channels-last rows [n*hw][ld]
__global__ void image_to_tokens_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, int n, int c, int hw) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)n * hw * c) return;
  const int ch = (int)(i % c);
  const long px = i / c;
  const int img = (int)(px / hw), p = (int)(px % hw);
  out[i] = x[((long)img * c + ch) * hw + p];
}
__global__ void tokens_to_image_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, int n, int c, int hw, int ld) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)n * c * hw) return;
  const int p = (int)(i % hw);
  const long t = i / hw;
  const int ch = (int)(t % c), img = (int)(t / c);
  out[i] = x[((long)img * hw + p) * ld + ch];
}

// DiagonalGaussianDistribution.sample() on fp16 tensors, one rounding per eager op: std = exp(0.5 * clamp(logvar, -30, 20));
// x = mean + std * noise
__global__ void gaussian_sample_kernel(const half_t* __restrict__ mean, const half_t* __restrict__ logvar,
                                       const half_t* __restrict__ noise, half_t* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float lv0 = (float)logvar[i];
  const float lv = lv0 != lv0 ? lv0 : fminf(fmaxf(lv0, -30.0f), 20.0f);  // torch.clamp keeps a NaN, fmaxf / fminf drop it
  const float sd = r16(expf(r16(0.5f * lv)));
  out[i] = (half_t)((float)mean[i] + r16(sd * (float)noise[i]));
}
// python-float x fp16 tensor (fp32 product rounded to fp32, then to fp16: the pinned VGPR keeps hipcc from fusing the two)
__global__ void scale_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, long n, float s) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float p = s * (float)x[i];
  asm volatile("" : "+v"(p));
  out[i] = (half_t)p;
}

extern "C" int mvoc_gaussian_sample_f16(const void* mean, const void* logvar, const void* noise, void* out, int64_t n, void* stream) {
  MVOC_REQUIRE(mean && logvar && noise && out && n > 0, -1, "gaussian_sample: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 8.0 * n);
  hipLaunchKernelGGL(gaussian_sample_kernel, dim3(nblk(n)), dim3(256), 0, s, (const half_t*)mean, (const half_t*)logvar,
                     (const half_t*)noise, (half_t*)out, (long)n);
  return mvoc_check_launch("gaussian_sample_kernel");
}

extern "C" int mvoc_clip_patches_f16(const void* pixels, void* out, int32_t nimg, int32_t size, int32_t patch, int32_t kpad,
                                     void* stream) {
  MVOC_REQUIRE(pixels && out && nimg > 0 && patch > 0 && size > 0 && size % patch == 0 && kpad >= 3 * patch * patch, -1,
               "clip_patches: bad args");
  const long total = (long)nimg * (size / patch) * (size / patch) * kpad;
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 4.0 * total);
  hipLaunchKernelGGL(clip_patches_kernel, dim3(nblk(total)), dim3(256), 0, s, (const half_t*)pixels, (half_t*)out, size, patch, kpad, total);
  return mvoc_check_launch("clip_patches_kernel");
}

extern "C" int mvoc_clip_embed_f16(const void* table, const int32_t* ids, const void* cls, const void* pos, void* out, int64_t rows,
                                   int32_t t, int32_t c, void* stream) {
  MVOC_REQUIRE(table && pos && out && rows > 0 && t > 0 && rows % t == 0 && c > 0 && c % 8 == 0 && (ids || cls), -1,
               "clip_embed: bad args (c %% 8, rows %% t, ids or cls)");
  // the kernel moves rows as 16-byte vectors: refuse, like softmax_rows, what they cannot address
  MVOC_REQUIRE((((uintptr_t)table | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)out) & 15) == 0, -1,
               "clip_embed: table, cls, pos and out must be 16-byte aligned");
  const long total = rows * (c / 8);
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 6.0 * rows * c);
  hipLaunchKernelGGL(clip_embed_kernel, dim3(nblk(total)), dim3(256), 0, s, (const half_t*)table, (const int*)ids, (const half_t*)cls,
                     (const half_t*)pos, (half_t*)out, t, c / 8, total);
  return mvoc_check_launch("clip_embed_kernel");
}

extern "C" int mvoc_scale_f16(const void* x, void* out, int64_t n, double scale, void* stream) {
  MVOC_REQUIRE(x && out && n > 0, -1, "scale: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 4.0 * n);
  hipLaunchKernelGGL(scale_kernel, dim3(nblk(n)), dim3(256), 0, s, (const half_t*)x, (half_t*)out, (long)n, (float)scale);
  return mvoc_check_launch("scale_kernel");
}

extern "C" int mvoc_conv1x1_small_f16(const void* x, const void* w, const void* bias, void* out, int64_t rows, int32_t cin,
                                      int32_t cout, void* stream) {
  MVOC_REQUIRE(x && w && out && rows > 0 && cin > 0 && cout > 0 && cin <= 64 && cout <= 64, -1, "conv1x1_small: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * rows * (cin + cout));
  hipLaunchKernelGGL(conv1x1_small_kernel, dim3(nblk(rows * cout)), dim3(256), 0, s, (const half_t*)x, (const half_t*)w,
                     (const half_t*)bias, (half_t*)out, (long)rows, cin, cout);
  return mvoc_check_launch("conv1x1_small_kernel");
}

extern "C" int mvoc_image_to_tokens_f16(const void* x, void* out, int32_t n, int32_t c, int32_t hw, void* stream) {
  MVOC_REQUIRE(x && out && n > 0 && c > 0 && hw > 0, -1, "image_to_tokens: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 4.0 * n * c * hw);
  hipLaunchKernelGGL(image_to_tokens_kernel, dim3(nblk((long)n * c * hw)), dim3(256), 0, s, (const half_t*)x, (half_t*)out, n, c, hw);
  return mvoc_check_launch("image_to_tokens_kernel");
}

extern "C" int mvoc_tokens_to_image_f16(const void* x, void* out, int32_t n, int32_t c, int32_t hw, int32_t ld, void* stream) {
  MVOC_REQUIRE(x && out && n > 0 && c > 0 && hw > 0 && ld >= c, -1, "tokens_to_image: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 4.0 * n * c * hw);
  hipLaunchKernelGGL(tokens_to_image_kernel, dim3(nblk((long)n * c * hw)), dim3(256), 0, s, (const half_t*)x, (half_t*)out, n, c, hw, ld);
  return mvoc_check_launch("tokens_to_image_kernel");
}

// ---- mask preprocessing on the device (reference utils.py:92-154) ----------------------------------------
// PIL's Image.resize (BICUBIC, 8-bit path) is integer arithmetic once its coefficient tables exist: per output index a window
// [xmin, xmin+n) and n fixed-point weights (22 fractional bits); acc = 2^21 + sum(pixel * w); out = clip8(acc >> 22).  The
// horizontal pass runs first and is itself rounded to uint8, then the vertical pass.  One thread per output pixel of a pass.
// in [n][len_o][len_i] (ALONG = innermost) or [n][len_i][len_o] viewed through (stride_i, stride_o).
__global__ void resize8_pass_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int* __restrict__ bounds,
                                    const int* __restrict__ kk, int ksize, long nimg, int olen, int other, long in_img, long out_img,
                                    long in_si, long in_so, long out_si, long out_so) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nimg * olen * other) return;
  const int xx = (int)(i % olen);
  const long t = i / olen;
  const int o = (int)(t % other);
  const long img = t / other;
  const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
  const uint8_t* src = in + img * in_img + (long)o * in_so + (long)xmin * in_si;
  int acc = 1 << 21;
  for (int x = 0; x < n; ++x) acc += (int)src[(long)x * in_si] * kk[xx * ksize + x];
  acc >>= 22;
  out[img * out_img + (long)o * out_so + (long)xx * out_si] = (uint8_t)(acc < 0 ? 0 : acc > 255 ? 255 : acc);
}
// float mask = v / 255 (fp32 division, one rounding to fp16: `.to(float32).div_(255.0).to(dtype)`), bool mask = v > 10
// (cv.threshold(v, 10, 255, THRESH_BINARY) -> {0, 255} -> / 255 -> bool)
__global__ void mask_finish_kernel(const uint8_t* __restrict__ v, half_t* __restrict__ fl, uint8_t* __restrict__ bl, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = v[i];
  fl[i] = (half_t)((float)x / 255.0f);
  bl[i] = x > 10 ? 1 : 0;
}

extern "C" int mvoc_mask_resize_u8(const void* in, void* tmp, void* out, int32_t n, int32_t H, int32_t W, int32_t h, int32_t w,
                                   const int32_t* bounds_h, const int32_t* kk_h, int32_t ksize_h, const int32_t* bounds_v,
                                   const int32_t* kk_v, int32_t ksize_v, void* stream) {
  MVOC_REQUIRE(in && tmp && out && bounds_h && kk_h && bounds_v && kk_v && n > 0 && H > 0 && W > 0 && h > 0 && w > 0, -1, "mask_resize: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, (double)n * H * W + 2.0 * n * H * w + (double)n * h * w);
  // horizontal: [n][H][W] -> tmp [n][H][w]
  hipLaunchKernelGGL(resize8_pass_kernel, dim3(nblk((long)n * H * w)), dim3(256), 0, s, (const uint8_t*)in, (uint8_t*)tmp, bounds_h, kk_h,
                     ksize_h, (long)n, w, H, (long)H * W, (long)H * w, 1L, (long)W, 1L, (long)w);
  // vertical: tmp [n][H][w] -> out [n][h][w]
  hipLaunchKernelGGL(resize8_pass_kernel, dim3(nblk((long)n * h * w)), dim3(256), 0, s, (const uint8_t*)tmp, (uint8_t*)out, bounds_v, kk_v,
                     ksize_v, (long)n, h, w, (long)H * w, (long)h * w, (long)w, 1L, (long)w, 1L);
  return mvoc_check_launch("resize8_pass_kernel");
}

extern "C" int mvoc_mask_finish(const void* v, void* float_mask, void* bool_mask, int64_t n, void* stream) {
  MVOC_REQUIRE(v && float_mask && bool_mask && n > 0, -1, "mask_finish: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 4.0 * n);
  hipLaunchKernelGGL(mask_finish_kernel, dim3(nblk(n)), dim3(256), 0, s, (const uint8_t*)v, (half_t*)float_mask, (uint8_t*)bool_mask, (long)n);
  return mvoc_check_launch("mask_finish_kernel");
}

// row permutation copy (frame shard <-> pixel shard packing around the RCCL exchanges): out rows are contiguous over the index
// (i0,i1,i2,i3); the source row of each is i0*s0 + i1*s1 + i2*s2 + i3*s3; thread = 16-byte chunk of a row
__global__ void permute_rows_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, int d1, int d2, int d3, long s0, long s1,
                                    long s2, long s3, int c8n, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c8 = (int)(i % c8n);
  long r = i / c8n;
  const int i3 = (int)(r % d3); r /= d3;
  const int i2 = (int)(r % d2); r /= d2;
  const int i1 = (int)(r % d1);
  const long i0 = r / d1;
  const long src = i0 * s0 + i1 * s1 + i2 * s2 + i3 * s3;
  reinterpret_cast<half8_t*>(out)[i] = *reinterpret_cast<const half8_t*>(x + (src * c8n + c8) * 8);
}

extern "C" int mvoc_permute_rows_f16(const void* x, void* out, const int64_t* dims4, const int64_t* strides4, int32_t c, void* stream) {
  MVOC_REQUIRE(x && out && dims4 && strides4 && c > 0 && c % 8 == 0, -1, "permute_rows: bad args (c %% 8)");
  MVOC_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, -1, "permute_rows: x and out must be 16-byte aligned");
  for (int k = 0; k < 4; ++k) MVOC_REQUIRE(dims4[k] > 0 && dims4[k] < (1 << 30), -1, "permute_rows: bad dim");
  const long total = (long)dims4[0] * dims4[1] * dims4[2] * dims4[3] * (c / 8);
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 32.0 * total);
  hipLaunchKernelGGL(permute_rows_kernel, dim3(nblk(total)), dim3(256), 0, s, (const half_t*)x, (half_t*)out, (int)dims4[1], (int)dims4[2],
                     (int)dims4[3], (long)strides4[0], (long)strides4[1], (long)strides4[2], (long)strides4[3], c / 8, total);
  return mvoc_check_launch("permute_rows_kernel");
}

extern "C" int mvoc_adaptive_avgpool_f16(const void* x, void* out, int32_t nimg, int32_t h, int32_t w, int32_t c,
                                         int32_t oh, int32_t ow, void* stream) {
  MVOC_REQUIRE(x && out && nimg > 0 && h > 0 && w > 0 && c > 0 && oh > 0 && ow > 0, -1, "avgpool: bad args");
  const long total = (long)nimg * oh * ow * c;
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 2.0 * ((double)nimg * h * w * c + total));
  hipLaunchKernelGGL(avgpool_kernel, dim3(nblk(total)), dim3(256), 0, s, (const half_t*)x, (half_t*)out, nimg, h, w, c, oh,
                     ow);
  return mvoc_check_launch("avgpool_kernel");
}

extern "C" int mvoc_ncfhw_to_tokens_f16(const void* x, void* out, int32_t b, int32_t c, int32_t f, int32_t hw, int32_t ldo,
                                        int32_t coff, void* stream) {
  MVOC_REQUIRE(x && out && b > 0 && c > 0 && f > 0 && hw > 0 && coff >= 0 && ldo >= coff + c, -1, "ncfhw_to_tokens: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 4.0 * b * c * f * hw);
  hipLaunchKernelGGL(ncfhw_to_tokens_kernel, dim3(nblk((long)b * f * hw)), dim3(256), 0, s, (const half_t*)x,
                     (half_t*)out, b, c, f, hw, ldo, coff);
  return mvoc_check_launch("ncfhw_to_tokens_kernel");
}

extern "C" int mvoc_tokens_to_ncfhw_f16(const void* x, void* out, int32_t b, int32_t c, int32_t f, int32_t hw, int32_t ld,
                                        void* stream) {
  MVOC_REQUIRE(x && out && b > 0 && c > 0 && f > 0 && hw > 0 && ld >= c, -1, "tokens_to_ncfhw: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 4.0 * b * c * f * hw);
  hipLaunchKernelGGL(tokens_to_ncfhw_kernel, dim3(nblk((long)b * c * f * hw)), dim3(256), 0, s, (const half_t*)x,
                     (half_t*)out, b, c, f, hw, ld);
  return mvoc_check_launch("tokens_to_ncfhw_kernel");
}

extern "C" int mvoc_temporal_encoder4_f16(const void* x, const void* params, void* out, int32_t b, int32_t f, int32_t hw,
                                          int32_t ldo, int32_t coff, void* stream) {
  MVOC_REQUIRE(x && params && out && b > 0 && f > 0 && hw > 0 && coff >= 0 && ldo >= coff + 4, -1, "temporal_encoder4: bad args");
  hipStream_t s = (hipStream_t)stream;
  MvocProfScope prof(MVOC_FAM_MISC, s, 16.0 * b * f * hw);
  hipLaunchKernelGGL(temporal_encoder4_kernel, dim3(nblk((long)b * f * hw)), dim3(256), 0, s, (const half_t*)x,
                     (const Enc4Params*)params, (half_t*)out, b, f, hw, ldo, coff);
  return mvoc_check_launch("temporal_encoder4_kernel");
}

extern "C" int mvoc_delay_us(int64_t us, void* stream) {
  MVOC_REQUIRE(us >= 0 && us <= 2000000, -1, "delay_us: out of range");
  hipLaunchKernelGGL(delay_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long)us * 100);
  return mvoc_check_launch("delay_kernel");
}
