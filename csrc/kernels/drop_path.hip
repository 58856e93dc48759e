// Stochastic depth (drop path) for gfx950: a residual branch is kept or dropped per SAMPLE.  The keep decision of
// sample b at a site is dropout's element definition (philox.h) with element index = sample index:
//   group g = b >> 3, one Philox4x32-10 call of (key, g), u = draw16(words, b & 7), kept iff u >= thr,
//   scale = 65536 / (65536 - thr).
//
//   pdt_drop_path_scales   keys [sites] (int64, DEVICE memory: a captured graph sees each replay's fresh keys),
//                          thr_scale [2, sites] fp32 (row 0 thr, row 1 scale)  ->  out [sites, B] fp32 of 0 | scale.
//                          Every consumer (the scaled window norm of norms.hip, the scaled fused MLP of
//                          swin_mlp.hip, the kernel below) takes one row of it: Philox stays out of the MFMA kernels.
//   pdt_drop_path_rows     y = (res ? res : 0) + (sc[b] != 0 ? x * sc[b] : 0), b = element / per_sample, over a
//                          contiguous tensor whose samples are `per_sample` consecutive elements (rows_per_sample
//                          * N).  A dropped sample is selected away, never multiplied by 0: inf / NaN in its branch
//                          do not reach y, and res passes bit for bit.  Forward and backward are the same map.
#include "common.h"
#include "philox.h"

using namespace pdt;

namespace {

constexpr int NT = 256;

__global__ __launch_bounds__(NT) void drop_path_scales_kernel(const int64_t* __restrict__ keys,
                                                              const float* __restrict__ thr_scale,
                                                              float* __restrict__ out, int sites, int B) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= sites * B) return;
  const int site = i / B, b = i - site * B;
  const uint64_t k = (uint64_t)keys[site];
  const uint32_t thr = (uint32_t)thr_scale[site];
  const philox::Words w = philox::group_words((uint64_t)(b >> 3), (uint32_t)k, (uint32_t)(k >> 32));
  out[i] = philox::draw16(w, b & 7) >= thr ? thr_scale[sites + site] : 0.f;
}

template <typename T> struct VecW;                       // elements per 16-byte vector
template <> struct VecW<float> { static constexpr int n = 4; };
template <> struct VecW<bf16_t> { static constexpr int n = 8; };

template <typename T, int V>
__device__ __forceinline__ void ld_vec(const T* p, float* o) {
  if constexpr (V == 8) Vec8<T>::load(p, o);
  else {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = v[j];
  }
}
template <typename T, int V>
__device__ __forceinline__ void st_vec(T* p, const float* o) {
  if constexpr (V == 8) Vec8<T>::store(p, o);
  else *reinterpret_cast<f32x4*>(p) = f32x4{o[0], o[1], o[2], o[3]};
}

// x * sc and the add are rounded separately: the torch composite computes exactly this, so the two agree bit for bit
// (hence this file is built with -ffp-contract=off: _build.PER_FILE_FLAGS; the backend fuses under the build's
// default -ffp-contract=fast whatever a pragma says)
__device__ __forceinline__ float scaled_add(float res, float x, float sc) {
  const float p = x * sc;
  return sc != 0.f ? res + p : res;
}

template <typename T, bool RES>
__global__ __launch_bounds__(NT) void drop_path_rows_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                            T* __restrict__ y, int64_t numel, int64_t per_sample,
                                                            const float* __restrict__ sc) {
  constexpr int V = VecW<T>::n;
  const int64_t vecs = numel / V;
  const int64_t stride = (int64_t)gridDim.x * NT;
  const bool narrow = numel < ((int64_t)1 << 32);         // 32-bit division where the element index fits
  for (int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x; g < vecs; g += stride) {
    const int64_t e0 = g * V;
    const int64_t b0 = narrow ? (int64_t)((uint32_t)e0 / (uint32_t)per_sample) : e0 / per_sample;
    const int64_t left = (b0 + 1) * per_sample - e0;      // elements of this vector's first sample from e0 on
    float s[V];
    if (left >= V) {
      const float s0 = sc[b0];
#pragma unroll
      for (int j = 0; j < V; ++j) s[j] = s0;
    } else {                                              // the vector straddles samples (per_sample % V != 0)
#pragma unroll
      for (int j = 0; j < V; ++j) s[j] = sc[j < left ? b0 : (e0 + j) / per_sample];
    }
    float r[V], o[V];
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = 0.f;
    if constexpr (RES) ld_vec<T, V>(res + e0, r);
    bool any = false;
#pragma unroll
    for (int j = 0; j < V; ++j) any |= s[j] != 0.f;
    if (any) {
      float v[V];
      ld_vec<T, V>(x + e0, v);
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = scaled_add(r[j], v[j], s[j]);
    } else {                                              // all dropped: x is not read
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = r[j];
    }
    st_vec<T, V>(y + e0, o);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int64_t e = vecs * V; e < numel; ++e) {
      const float s0 = sc[e / per_sample];
      const float r0 = RES ? to_f<T>(res[e]) : 0.f;
      y[e] = from_f<T>(s0 != 0.f ? scaled_add(r0, to_f<T>(x[e]), s0) : r0);
    }
  }
}

template <typename T>
int launch_rows(const void* x, const void* res, void* y, int64_t numel, int64_t per_sample, const float* sc,
                hipStream_t st) {
  const int grid = grid_for(numel / VecW<T>::n, NT, 256 * 16);
  if (res)
    drop_path_rows_kernel<T, true><<<grid, NT, 0, st>>>((const T*)x, (const T*)res, (T*)y, numel, per_sample, sc);
  else
    drop_path_rows_kernel<T, false><<<grid, NT, 0, st>>>((const T*)x, nullptr, (T*)y, numel, per_sample, sc);
  return (int)hipGetLastError();
}

}  // namespace

// out [sites, B] = 0 | scale of each (site, sample); keys [sites] int64 and thr_scale [2, sites] fp32 on the device
PDT_API int pdt_drop_path_scales(const void* keys, const float* thr_scale, float* out, int sites, int B,
                                 hipStream_t st) {
  if (sites <= 0 || B <= 0 || (int64_t)sites * B > (1 << 30) || !keys || !thr_scale || !out)
    return (int)hipErrorInvalidValue;
  drop_path_scales_kernel<<<(sites * B + NT - 1) / NT, NT, 0, st>>>((const int64_t*)keys, thr_scale, out, sites, B);
  return (int)hipGetLastError();
}

// y = (res ? res : 0) + (sc[b] != 0 ? x * sc[b] : 0) over numel elements, b = element / per_sample; sc holds
// numel / per_sample fp32 scales; x / res / y 16-byte aligned; dt in {kF32, kBF16}
PDT_API int pdt_drop_path_rows(const void* x, const void* res, void* y, int64_t numel, int64_t per_sample,
                               const float* sc, int dt, hipStream_t st) {
  if (numel <= 0 || per_sample <= 0 || numel % per_sample != 0 || !sc ||
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(y)) & 15))
    return (int)hipErrorInvalidValue;
  if (dt == kBF16) return launch_rows<bf16_t>(x, res, y, numel, per_sample, sc, st);
  if (dt == kF32) return launch_rows<float>(x, res, y, numel, per_sample, sc, st);
  return (int)hipErrorInvalidValue;
}
