// Elementwise passes over flat buffers (casts, scale, the FGSM step, the backward of VLFusion's concat + dropout, the dropout-mask probe
// used by tests, the RNG advance) and the library's ABI version.  All HBM-bound: 16-byte vector accesses where the layout allows.
#include "common.h"

// out = x + eps * sign(g) (evaluate_gen_attack.py:131), sign(+-0) = 0 as torch.sign has it; sign(NaN) = NaN.  The sign is read off
// the bits, so a denormal g counts whatever the denormal mode.  out may be x: every element is read and written by one thread.
DEVFN float fgsm_one(float x, float g, float eps) {
#pragma clang fp contract(off)
  const uint32_t b = __builtin_bit_cast(uint32_t, g), mag = b & 0x7fffffffu;
  const float s = mag == 0u ? 0.f : (mag > 0x7f800000u ? g : ((b >> 31) ? -1.f : 1.f));
  return x + eps * s;
}
__global__ __launch_bounds__(256) void fgsm_step_kernel(const float* x, const float* g, float eps, float* out, int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 3 < n) {
    const f32x4 xv = ld4(x + i), gv = ld4(g + i);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fgsm_one(xv[e], gv[e], eps);
    st4(out + i, o);
  } else {
    for (int64_t j = i; j < n; ++j) out[j] = fgsm_one(x[j], g[j], eps);
  }
}

template <typename S, typename Dt>
__global__ __launch_bounds__(256) void cast_kernel(const S* src, Dt* dst, int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 3 < n) st4(dst + i, ld4(src + i));
  else for (int64_t j = i; j < n; ++j) dst[j] = from_f<Dt>(to_f(src[j]));
}

// fp32 -> bf16 over a LIST of ranges of two flat buffers with the same indexing (gstvd_cast_ranges): block b serves 1024 elements
// of the range whose block interval [blk0[i], blk0[i + 1]) holds it
__global__ __launch_bounds__(256) void cast_ranges_kernel(const float* src, bf16* dst, const int64_t* tab, const int32_t* blk0, int n) {
  const int b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (blk0[mid] <= b) lo = mid; else hi = mid - 1; }
  const int64_t start = tab[2 * lo], len = tab[2 * lo + 1];
  const int64_t i = ((int64_t)(b - blk0[lo]) * 256 + threadIdx.x) * 4;
  if (i + 3 < len) st4(dst + start + i, ld4(src + start + i));
  else for (int64_t j = i; j < len; ++j) dst[start + j] = (bf16)src[start + j];
}

__global__ void scale_kernel(float* x, const float* f, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] *= f[0];
}
__global__ void rng_advance_kernel(uint64_t* rng) { rng[1] += 1; }
__global__ void dropout_mask_kernel(float* out, int64_t n, float p, uint32_t site, const uint64_t* rng) {
  const DropKey dk = make_drop(p, site, rng);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = drop_factor(dk, (uint64_t)i);
}

// backward of VLFusion's concat + dropout (visual_dialog_model.py:132-133): split d_enc[B, R+T, H] into the
// vision rows [B*R, H] and the text rows [B*T, H], re-applying each half's dropout mask
template <typename T>
__global__ __launch_bounds__(256) void vl_split_kernel(const T* d, int64_t B, int64_t R, int64_t Tt, int64_t H, T* dv, T* dt_,
                                                       float p, uint32_t site_v, uint32_t site_t, const uint64_t* rng) {
  const DropKey kv = make_drop(p, site_v, rng), kt = make_drop(p, site_t, rng);
  const int64_t S = R + Tt, H4 = H / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * S * H4) return;
  const int64_t c = (i % H4) * 4, row = i / H4, b = row / S, r = row % S;
  f32x4 v = ld4(d + row * H + c);
  if (r < R) { const int64_t o = (b * R + r) * H + c; st4(dv + o, v * drop_factor4(kv, (uint64_t)o)); }
  else { const int64_t o = (b * Tt + (r - R)) * H + c; st4(dt_ + o, v * drop_factor4(kt, (uint64_t)o)); }
}

// ---- C ABI ----------------------------------------------------------------------------------------------
// 2: gstvd_ln_bwd_t.nblk (round 2); 3: gstvd_gemm_ln_fwd / _bwd, debug entry gone (round 3); 4: gstvd_gemm_grouped_adamw,
// gstvd_adamw_blocks (round 4); 5: block_map_dev / nblocks of the grouped launches (round 5); 6-9: DESIGN.md
// (entry points added without a signature change do not bump it: gstvd_rows_* / gstvd_kl_*, gstvd_ln_kernel_name)
extern "C" int gstvd_abi_version(void) { return 9; }
extern "C" const char* gstvd_build_arch(void) { return "gfx950"; }

extern "C" int gstvd_vl_split(const void* d_enc, int64_t B, int64_t R, int64_t T, int64_t H, int32_t dtype, void* d_v, void* d_t,
                              float p, uint32_t site_v, uint32_t site_t, const uint64_t* rng, gstvd_stream_t stream) {
  if (!d_enc || !d_v || !d_t) return GSTVD_E_NULL;
  if (B <= 0 || R <= 0 || T <= 0 || H <= 0 || (H % 4)) return GSTVD_E_SHAPE;
  dim3 grid((unsigned)((B * (R + T) * (H / 4) + 255) / 256));
  GSTVD_FOR_DTYPE(dtype, E, hipLaunchKernelGGL(vl_split_kernel<E>, grid, dim3(256), 0, (hipStream_t)stream, (const E*)d_enc, B, R, T, H, (E*)d_v, (E*)d_t, p, site_v, site_t, rng));
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_fgsm_step(const float* x, const float* g, float eps, float* out, int64_t n, gstvd_stream_t stream) {
  if (!x || !g || !out) return GSTVD_E_NULL;
  if (n <= 0 || n > ((int64_t)1 << 40)) return GSTVD_E_SHAPE;
  if (((uintptr_t)x | (uintptr_t)g | (uintptr_t)out) & 15) return GSTVD_E_ALIGN;
  hipLaunchKernelGGL(fgsm_step_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, x, g, eps, out, n);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_cast(const void* src, int32_t sdt, void* dst, int32_t ddt, int64_t n, gstvd_stream_t stream) {
  if (!src || !dst) return GSTVD_E_NULL;
  if (n <= 0) return GSTVD_E_SHAPE;
  if (((uintptr_t)src | (uintptr_t)dst) & 15) return GSTVD_E_ALIGN;
  dim3 grid((unsigned)((n + 1023) / 1024));
  GSTVD_FOR_DTYPE(sdt, S, GSTVD_FOR_DTYPE(ddt, D, hipLaunchKernelGGL((cast_kernel<S, D>), grid, dim3(256), 0, (hipStream_t)stream, (const S*)src, (D*)dst, n)));
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_cast_ranges(const float* src, void* dst_bf16, const int64_t* ranges_dev, const int32_t* blk0_dev, int64_t nranges,
                                 int64_t total_blocks, gstvd_stream_t stream) {
  if (!src || !dst_bf16 || !ranges_dev || !blk0_dev) return GSTVD_E_NULL;
  if (nranges <= 0 || total_blocks <= 0 || nranges > (1 << 24)) return GSTVD_E_SHAPE;
  if (((uintptr_t)src & 15) || ((uintptr_t)dst_bf16 & 7)) return GSTVD_E_ALIGN;
  hipLaunchKernelGGL(cast_ranges_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, src, (bf16*)dst_bf16, ranges_dev, blk0_dev,
                     (int)nranges);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_scale(float* x, const float* factor, int64_t n, gstvd_stream_t stream) {
  if (!x || !factor) return GSTVD_E_NULL;
  if (n <= 0) return GSTVD_E_SHAPE;
  hipLaunchKernelGGL(scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, factor, n);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
extern "C" int gstvd_rng_advance(uint64_t* rng, gstvd_stream_t stream) {
  if (!rng) return GSTVD_E_NULL;
  hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, rng);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
extern "C" int gstvd_dropout_mask(float* out, int64_t n, float p, uint32_t site, const uint64_t* rng, gstvd_stream_t stream) {
  if (!out || !rng) return GSTVD_E_NULL;
  if (n <= 0) return GSTVD_E_SHAPE;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, n, p, site, rng);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
