// vits_expand_prior: the prior expansion of SynthesizerTrn.infer (models.py:507-520) in one launch.
//
// Eager composition it replaces (per item):
//   w_ceil = ceil(exp(logw) * x_mask * length_scale)   |   durations * x_mask
//   y_len  = max(sum(w_ceil), 1)
//   path   = generate_path(w_ceil, mask)                       dense one-hot [t_y][t_x]
//   m, logs = path @ m_p^T, path @ logs_p^T                    two GEMMs (exact: one 1 per row)
//   z_p    = m + eps * exp(logs) * noise_scale
// Here: the durations' inclusive prefix sum in LDS, then per frame t the token upper_bound(cum, t) and a gather of its row.
//
// Rounding follows the eager ops one by one: expf / ceilf (the routines torch's element-wise kernels call), every product and
// sum rounded separately to fp32 (no fma contraction).  Under bf16 autocast the GEMMs return m and logs rounded to bf16 and the
// noise is drawn in bf16 (randn_like of the GEMM output), but exp runs in fp32 (autocast's fp32 list) and the bf16 x fp32
// products promote to fp32: z_p is fp32 in both modes, only the inputs differ (TE = bf16 rounds m and logs first).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFrames = 16;        // frame rows per workgroup
constexpr int kVec = 8;            // channels per thread and access: 2 x 16 B (fp32) or 1 x 16 B (bf16)

__device__ __forceinline__ void load8(const float* p, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void load8(const __bf16* p, float* v) {
  const uint4 a = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ void store8(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
template <typename T> __device__ __forceinline__ float rnd(float f) { return f; }
template <> __device__ __forceinline__ float rnd<__bf16>(float f) { return (float)(__bf16)f; }

// grid (max(1, ceil(t_cap / kFrames)), b); dynamic LDS: cum[t_x] floats.  Every workgroup redoes its item's scan (t_x values,
// as generate_path_kernel does); workgroup x = 0 also writes w_ceil and y_lengths.
template <typename TS, typename TE>
__global__ __launch_bounds__(kThreads) void expand_prior_kernel(const float* __restrict__ logw, const float* __restrict__ dur,
                                                                const int64_t* __restrict__ x_lengths, const TS* __restrict__ m,
                                                                long ld_row, long ld_batch, int logs_off, const TE* __restrict__ eps,
                                                                const float* __restrict__ scalars, float* __restrict__ z_p,
                                                                float* __restrict__ y_mask, int* __restrict__ y_lengths,
                                                                int* __restrict__ w_ceil, int t_x, int t_cap, int C) {
#pragma clang fp contract(off)
  extern __shared__ float cum[];                // [t_x]
  __shared__ float carry_s, wave_tot[kThreads / 64];
  __shared__ int tok_s[kFrames];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long x_len = x_lengths[b];
  const float length_scale = scalars[0], noise_scale = scalars[1];
  if (tid == 0) carry_s = 0.f;
  __syncthreads();
  for (int x0 = 0; x0 < t_x; x0 += kThreads) {
    const int x = x0 + tid;
    float v = 0.f;
    if (x < t_x) {
      const float mask = x < x_len ? 1.f : 0.f;
      v = dur ? dur[(size_t)b * t_x + x] * mask : ceilf(expf(logw[(size_t)b * t_x + x]) * mask * length_scale);
      if (blockIdx.x == 0) w_ceil[(size_t)b * t_x + x] = (int)v;
    }
    for (int o = 1; o < 64; o <<= 1) {          // inclusive scan inside the wave
      const float u = __shfl_up(v, o, 64);
      if ((tid & 63) >= o) v += u;
    }
    if ((tid & 63) == 63) wave_tot[tid >> 6] = v;
    __syncthreads();
    float base = carry_s;
    for (int w = 0; w < (tid >> 6); ++w) base += wave_tot[w];
    if (x < t_x) cum[x] = v + base;
    __syncthreads();
    if (tid == 0) carry_s += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    __syncthreads();
  }
  const float total = carry_s;
  const int y_len = total > 1.f ? (int)total : 1;                    // clamp_min(sum(w_ceil), 1).long()
  if (blockIdx.x == 0 && tid == 0) y_lengths[b] = y_len;
  const int f0 = blockIdx.x * kFrames;
  if (f0 >= t_cap) return;
  if (tid < kFrames) {
    const int t = f0 + tid;
    int lo = 0, hi = t_x;                       // first x with t < cum[x] (t_x: no token covers t)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((float)t < cum[mid]) hi = mid; else lo = mid + 1;
    }
    tok_s[tid] = lo;
    if (t < t_cap) y_mask[(size_t)b * t_cap + t] = t < y_len ? 1.f : 0.f;
  }
  __syncthreads();
  const int nv = C / kVec;
  for (int i = tid; i < kFrames * nv; i += kThreads) {
    const int f = i / nv, c = (i - f * nv) * kVec, t = f0 + f;
    if (t >= t_cap) break;                      // rows are walked in order: the rest are past t_cap too
    const size_t o = ((size_t)b * t_cap + t) * C + c;
    float z[kVec];
    if (t >= y_len) {
#pragma unroll
      for (int k = 0; k < kVec; ++k) z[k] = 0.f;
    } else {
      const int j = tok_s[f];
      float mv[kVec], lv[kVec], ev[kVec];
      if (j < t_x) {
        const TS* row = m + (size_t)b * ld_batch + (size_t)j * ld_row + c;
        load8(row, mv);
        load8(row + logs_off, lv);
      } else {                                  // a frame no token covers (all durations zero): the path row is zero
#pragma unroll
        for (int k = 0; k < kVec; ++k) mv[k] = lv[k] = 0.f;
      }
      load8(eps + o, ev);
#pragma unroll
      for (int k = 0; k < kVec; ++k) {
        const float e = expf(rnd<TE>(lv[k]));
        const float a = ev[k] * e;
        const float s = a * noise_scale;
        z[k] = rnd<TE>(mv[k]) + s;
      }
    }
    store8(z_p + o, z);
  }
}

template <typename TS, typename TE>
int launch(const float* logw, const float* dur, const int64_t* x_lengths, const void* m, long ld_row, long ld_batch, int logs_off,
           const void* eps, const float* scalars, void* z_p, float* y_mask, int* y_lengths, int* w_ceil, int b, int t_x, int t_cap,
           int c, hipStream_t s) {
  const dim3 grid(t_cap > 0 ? vits::ceil_div(t_cap, kFrames) : 1, b);
  hipLaunchKernelGGL((expand_prior_kernel<TS, TE>), grid, dim3(kThreads), (size_t)t_x * 4, s, logw, dur, x_lengths,
                     static_cast<const TS*>(m), ld_row, ld_batch, logs_off, static_cast<const TE*>(eps), scalars,
                     static_cast<float*>(z_p), y_mask, y_lengths, w_ceil, t_x, t_cap, c);
  return vits::check_launch("vits_expand_prior");
}

}  // namespace

extern "C" int vits_expand_prior(int s_dtype, int eps_dtype, const float* logw, const float* durations, const int64_t* x_lengths,
                                 const void* m, long ld_row, long ld_batch, int logs_off, const void* eps, const float* scalars,
                                 void* z_p, float* y_mask, int* y_lengths, int* w_ceil, int b, int t_x, int t_cap, int c,
                                 void* stream) {
  if ((!logw && !durations) || !x_lengths || !scalars || !y_lengths || !w_ceil || b <= 0 || t_x <= 0 || t_cap < 0 || c < 0)
    return VITS_E_BADARG;
  if (t_cap > 0 && (c == 0 || !m || !eps || !z_p || !y_mask || ld_row < c || logs_off < c || ld_row < logs_off + c ||
                    ld_batch < (long)t_x * ld_row))
    return VITS_E_BADARG;
  if (b > 65535 || (size_t)t_x * 4 > 60 * 1024 || c % kVec != 0) return VITS_E_UNSUPPORTED;
  const bool sb = s_dtype == VITS_DT_BF16, ob = eps_dtype == VITS_DT_BF16;
  if ((!sb && s_dtype != VITS_DT_F32) || (!ob && eps_dtype != VITS_DT_F32)) return VITS_E_UNSUPPORTED;
  if (t_cap > 0) {                              // 16-byte accesses: aligned bases and row pitches
    const size_t es = sb ? 2 : 4;
    if ((reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(z_p)) % 16 != 0 ||
        ((size_t)ld_row * es) % 16 != 0 || ((size_t)ld_batch * es) % 16 != 0 || ((size_t)logs_off * es) % 16 != 0)
      return VITS_E_UNSUPPORTED;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
#define VITS_EXPAND(TS, TO) \
  launch<TS, TO>(logw, durations, x_lengths, m, ld_row, ld_batch, logs_off, eps, scalars, z_p, y_mask, y_lengths, w_ceil, b, t_x, t_cap, c, s)
  if (sb && ob) return VITS_EXPAND(__bf16, __bf16);
  if (sb) return VITS_EXPAND(__bf16, float);
  if (ob) return VITS_EXPAND(float, __bf16);
  return VITS_EXPAND(float, float);
#undef VITS_EXPAND
}
