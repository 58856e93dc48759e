// Dropout for gfx950 with no stored mask: the keep decision of element e is a pure function of (key, e)
// through Philox4x32-10 (philox.h), so the backward regenerates it.  The key is an int64 in DEVICE memory (a
// captured graph sees a fresh key on every replay); thr / scale come from the host:
//   thr = min(65535, round(p * 65536)), keep iff u16 >= thr, scale = 65536 / (65536 - thr).
//
//   pdt_dropout_fwd            y = keep ? x * scale : 0           (any numel: 16-byte vectors + a scalar tail)
//   pdt_dropout_bwd            dx = keep ? dy * scale : 0, optionally the column sums of dx AS STORED for a
//                              [rows, N] view (the gradient of a bias added in front of the mask), the same pass
//   pdt_dropout_add_norm_fwd   the fused residual site: s = x + drop(r + rb)  (mode 0, attention / MLP branch)
//                              or s = drop(x + r) (mode 1, the embedding sum), then (LayerNorm | RMSNorm)(s) --
//                              one wave per row, the row in registers, fp32 statistics over exactly the T-rounded
//                              s that is stored (the structure of norms.hip's norm_fwd_kernel, which stays as
//                              it is for the p = 0 path).
// One Philox call serves 8 consecutive elements = one 16-byte bf16 vector = one lane's share of a 512-column slab.
#include "common.h"
#include "philox.h"
#include "reduce.h"

using namespace pdt;

namespace {

constexpr int NT = 256;      // threads per block
constexpr int RPB = NT / 64; // rows per block of the fused kernel (one per wave)

struct Key {
  uint32_t k0, k1;
};
__device__ __forceinline__ Key read_key(const int64_t* __restrict__ key) {
  const uint64_t k = (uint64_t)*key;
  return Key{(uint32_t)k, (uint32_t)(k >> 32)};
}

// y = keep ? x * scale : 0 over numel elements (forward and backward are the same map)
template <typename T>
__global__ __launch_bounds__(NT) void dropout_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t numel,
                                                     const int64_t* __restrict__ key, uint32_t thr, float scale) {
  const Key k = read_key(key);
  const int64_t groups = numel >> 3;
  const int64_t stride = (int64_t)gridDim.x * NT;
  for (int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x; g < groups; g += stride) {
    float v[8];
    Vec8<T>::load(x + g * 8, v);
    const uint32_t keep = philox::group_keep((uint64_t)g, k.k0, k.k1, thr);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (keep >> j) & 1u ? v[j] * scale : 0.f;
    Vec8<T>::store(y + g * 8, v);
  }
  const int tail = (int)(numel & 7);
  if (tail != 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t keep = philox::group_keep((uint64_t)groups, k.k0, k.k1, thr);
    for (int j = 0; j < tail; ++j) {
      const int64_t e = groups * 8 + j;
      y[e] = from_f<T>((keep >> j) & 1u ? to_f<T>(x[e]) * scale : 0.f);
    }
  }
}

// dx = keep ? dy * scale : 0 for a [rows, N] matrix (N % 8 == 0, so a group never straddles two rows) plus one
// fp32 partial row of column sums of dx as stored per workgroup: reduce.h's (column group) x (row chunk) sweep.
template <typename T>
__global__ __launch_bounds__(NT) void dropout_bwd_colsum_kernel(const T* __restrict__ dy, T* __restrict__ dx, int rows,
                                                                int N, int rows_per, const int64_t* __restrict__ key,
                                                                uint32_t thr, float scale, float* __restrict__ part) {
  // blockIdx.x = 2048-column group (256 threads x 8 columns), blockIdx.y = row chunk
  const int col = (blockIdx.x * NT + threadIdx.x) * 8;
  if (col >= N) return;
  const Key k = read_key(key);
  const int r0 = blockIdx.y * rows_per;
  const int r1 = min(rows, r0 + rows_per);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = r0; r < r1; ++r) {
    const int64_t e = (int64_t)r * N + col;
    float v[8];
    Vec8<T>::load(dy + e, v);
    const uint32_t keep = philox::group_keep((uint64_t)e >> 3, k.k0, k.k1, thr);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = (keep >> j) & 1u ? v[j] * scale : 0.f;
      acc[j] += to_f<T>(from_f<T>(v[j]));
    }
    Vec8<T>::store(dx + e, v);
  }
  Vec8<float>::store(part + (int64_t)blockIdx.y * N + col, acc);
}

// narrow N (< 8 * NT): NT / (N / 8) rows per workgroup pass, folded through LDS in a fixed order
template <typename T>
__global__ __launch_bounds__(NT) void dropout_bwd_colsum_narrow(const T* __restrict__ dy, T* __restrict__ dx, int rows,
                                                                int N, int rows_per, const int64_t* __restrict__ key,
                                                                uint32_t thr, float scale, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float sacc[NT * 8];
  const Key k = read_key(key);
  const int tpr = N / 8, rpb = NT / tpr;
  const int rg = threadIdx.x / tpr, col = (threadIdx.x - rg * tpr) * 8;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int r0 = blockIdx.x * rows_per, r1 = min(rows, r0 + rows_per);
  if (rg < rpb) {
    for (int r = r0 + rg; r < r1; r += rpb) {
      const int64_t e = (int64_t)r * N + col;
      float v[8];
      Vec8<T>::load(dy + e, v);
      const uint32_t keep = philox::group_keep((uint64_t)e >> 3, k.k0, k.k1, thr);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[j] = (keep >> j) & 1u ? v[j] * scale : 0.f;
        acc[j] += to_f<T>(from_f<T>(v[j]));
      }
      Vec8<T>::store(dx + e, v);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) sacc[threadIdx.x * 8 + j] = acc[j];
  __syncthreads();
  for (int c = threadIdx.x; c < N; c += NT) {
    const int cv = c >> 3, j = c & 7;
    float t = 0.f;
    for (int g = 0; g < rpb; ++g) t += sacc[(g * tpr + cv) * 8 + j];
    part[(int64_t)blockIdx.x * N + c] = t;
  }
}

// The fused site.  MODE 0 (residual): s = x + drop(r + rb); a dropped element stores x's own bits.
// MODE 1 (sum): s = drop(x + r).  y = norm(s) over the T-rounded s.
template <typename T, typename W, int ITERS, bool RMS, int MODE>
__global__ __launch_bounds__(NT) void dropout_add_norm_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ res, const W* __restrict__ rb, T* __restrict__ sum_out,
    const W* __restrict__ w, const W* __restrict__ b, T* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int rows, int N, float eps, const int64_t* __restrict__ key, uint32_t thr,
    float scale) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float invN = 1.f / (float)N;
  const Key k = read_key(key);
  for (int row = blockIdx.x * RPB + wid; row < rows; row += gridDim.x * RPB) {
    const int64_t base = (int64_t)row * N;
    float v[ITERS][8];
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int col = it * 512 + lane * 8;
      if (col < N) {
        float r8[8];
        Vec8<T>::load(x + base + col, v[it]);
        Vec8<T>::load(res + base + col, r8);
        const uint32_t keep = philox::group_keep((uint64_t)(base + col) >> 3, k.k0, k.k1, thr);
        if constexpr (MODE == 0) {
          if (rb != nullptr) {
            float b8[8];
            Vec8<W>::load(rb + col, b8);
#pragma unroll
            for (int j = 0; j < 8; ++j) r8[j] += b8[j];
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) v[it][j] = (keep >> j) & 1u ? v[it][j] + r8[j] * scale : v[it][j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[it][j] = (keep >> j) & 1u ? (v[it][j] + r8[j]) * scale : 0.f;
        }
        Vec8<T>::store(sum_out + base + col, v[it]);
        // normalise exactly what was stored (the T-rounded sum), rounded in registers
        if constexpr (sizeof(T) == 2) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[it][j] = bf2f(f2bf(v[it][j]));
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[it][j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s += RMS ? v[it][j] * v[it][j] : v[it][j];
    }
    s = wave_sum(s);
    float mean = 0.f, rstd;
    if (RMS) {
      rstd = rsqrtf(s * invN + eps);
    } else {
      mean = s * invN;
      float q = 0.f;
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        const int col = it * 512 + lane * 8;
        if (col < N) {
#pragma unroll
          for (int j = 0; j < 8; ++j) { float d = v[it][j] - mean; q += d * d; }
        }
      }
      q = wave_sum(q);
      rstd = rsqrtf(q * invN + eps);
    }
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int col = it * 512 + lane * 8;
      if (col < N) {
        float wv[8], bv[8], o[8];
        Vec8<W>::load(w + col, wv);
        if (!RMS && b != nullptr) Vec8<W>::load(b + col, bv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float t = (v[it][j] - mean) * rstd * wv[j];
          o[j] = (!RMS && b != nullptr) ? t + bv[j] : t;
        }
        Vec8<T>::store(y + base + col, o);
      }
    }
    if (lane == 0) {
      if (mean_out) mean_out[row] = mean;
      rstd_out[row] = rstd;
    }
  }
}

template <typename T, typename W, bool RMS, int MODE>
int launch_site(const void* x, const void* res, const void* rb, void* sum_out, const void* w, const void* b, void* y,
                float* mean, float* rstd, int rows, int N, float eps, const int64_t* key, uint32_t thr, float scale,
                hipStream_t st) {
  const T* X = (const T*)x; const T* R = (const T*)res; T* S = (T*)sum_out; const W* RB = (const W*)rb;
  const W* Wt = (const W*)w; const W* B = (const W*)b; T* Y = (T*)y;
  // the grid of norms.hip's fused residual add (96 workgroups per CU), grid-stride over the rest
  const int grid = grid_for(rows, RPB, 256 * 96);
  const int iters = (N + 511) / 512;
#define PDT_DS(I)                                                                                                   \
  dropout_add_norm_fwd_kernel<T, W, I, RMS, MODE><<<grid, NT, 0, st>>>(X, R, RB, S, Wt, B, Y, mean, rstd, rows, N, \
                                                                        eps, key, thr, scale)
  if (iters <= 1) PDT_DS(1);
  else if (iters <= 2) PDT_DS(2);
  else PDT_DS(4);
#undef PDT_DS
  return (int)hipGetLastError();
}

template <typename T, typename W>
int dispatch_site(int rms, int mode, const void* x, const void* res, const void* rb, void* sum_out, const void* w,
                  const void* b, void* y, float* mean, float* rstd, int rows, int N, float eps, const int64_t* key,
                  uint32_t thr, float scale, hipStream_t st) {
#define PDT_ARGS x, res, rb, sum_out, w, b, y, mean, rstd, rows, N, eps, key, thr, scale, st
  if (rms) return mode ? launch_site<T, W, true, 1>(PDT_ARGS) : launch_site<T, W, true, 0>(PDT_ARGS);
  return mode ? launch_site<T, W, false, 1>(PDT_ARGS) : launch_site<T, W, false, 0>(PDT_ARGS);
#undef PDT_ARGS
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// x, y: dt in {kF32, kBF16}, contiguous, 16-byte aligned.  key: int64[1] in device memory.  0 <= thr <= 65535.
PDT_API int pdt_dropout_fwd(const void* x, void* y, int64_t numel, const int64_t* key, int thr, float scale, int dt,
                            hipStream_t st) {
  if (numel < 0 || thr < 0 || thr > 65535 || !key || !aligned16(x) || !aligned16(y)) return (int)hipErrorInvalidValue;
  if (numel == 0) return 0;
  const int grid = grid_for((numel + 7) / 8, NT);
  if (dt == kBF16) dropout_kernel<bf16_t><<<grid, NT, 0, st>>>((const bf16_t*)x, (bf16_t*)y, numel, key, thr, scale);
  else if (dt == kF32) dropout_kernel<float><<<grid, NT, 0, st>>>((const float*)x, (float*)y, numel, key, thr, scale);
  else return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

PDT_API int pdt_dropout_bwd_ws_floats(int rows, int N) { return (int)red::col_ws_floats(rows, N); }

// dx = keep ? dy * scale : 0.  colsum (nullable, cdt in {kF32, kBF16}, [N]): column sums of the stored dx for the
// [rows, N] view (rows * N == numel, N % 8 == 0); ws then holds pdt_dropout_bwd_ws_floats(rows, N) floats.
PDT_API int pdt_dropout_bwd(const void* dy, void* dx, int64_t numel, const int64_t* key, int thr, float scale, int dt,
                            void* colsum, int cdt, int rows, int N, float* ws, hipStream_t st) {
  if (!colsum) return pdt_dropout_fwd(dy, dx, numel, key, thr, scale, dt, st);
  if (thr < 0 || thr > 65535 || !key || !ws || rows <= 0 || N <= 0 || N % 8 != 0 || (int64_t)rows * N != numel ||
      !aligned16(dy) || !aligned16(dx) || (dt != kBF16 && dt != kF32) || (cdt != kBF16 && cdt != kF32))
    return (int)hipErrorInvalidValue;
  const red::ColPlan pl = red::col_plan(rows, N);
  if (N < 8 * NT) {
    if (dt == kBF16)
      dropout_bwd_colsum_narrow<bf16_t><<<pl.R, NT, 0, st>>>((const bf16_t*)dy, (bf16_t*)dx, rows, N, pl.rows_per, key,
                                                             thr, scale, ws);
    else
      dropout_bwd_colsum_narrow<float><<<pl.R, NT, 0, st>>>((const float*)dy, (float*)dx, rows, N, pl.rows_per, key,
                                                            thr, scale, ws);
  } else {
    const dim3 grid(pl.col_groups, pl.R);
    if (dt == kBF16)
      dropout_bwd_colsum_kernel<bf16_t><<<grid, NT, 0, st>>>((const bf16_t*)dy, (bf16_t*)dx, rows, N, pl.rows_per, key,
                                                             thr, scale, ws);
    else
      dropout_bwd_colsum_kernel<float><<<grid, NT, 0, st>>>((const float*)dy, (float*)dx, rows, N, pl.rows_per, key,
                                                            thr, scale, ws);
  }
  float* ws2 = ws + (int64_t)pl.R * N;
  if (cdt == kBF16) red::col_reduce<bf16_t>(ws, pl.R, N, (bf16_t*)colsum, ws2, 0, st);
  else red::col_reduce<float>(ws, pl.R, N, (float*)colsum, ws2, 0, st);
  return (int)hipGetLastError();
}

// The fused dropout + residual add + norm site.  x / res / sum_out / y: [rows, N] of xdt; w / b / res_bias: [N] of
// wdt; N % 8 == 0 and N <= 2048.  mode 0: sum_out = x + drop(res + res_bias); mode 1: sum_out = drop(x + res)
// (res_bias must be null).  rms = 1: RMSNorm (b ignored, mean unused).
PDT_API int pdt_dropout_add_norm_fwd(const void* x, const void* res, const void* res_bias, void* sum_out,
                                     const void* w, const void* b, void* y, float* mean, float* rstd, int rows, int N,
                                     float eps, const int64_t* key, int thr, float scale, int mode, int xdt, int wdt,
                                     int rms, hipStream_t st) {
  if (!x || !res || !sum_out || !w || !y || !rstd || !key || rows < 0 || N <= 0 || N % 8 != 0 || N > 2048 ||
      thr < 0 || thr > 65535 || (mode != 0 && mode != 1) || (mode == 1 && res_bias) || (!rms && !mean) ||
      !aligned16(x) || !aligned16(res) || !aligned16(sum_out) || !aligned16(y) || !aligned16(w) ||
      (b && !aligned16(b)) || (res_bias && !aligned16(res_bias)))
    return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
#define PDT_ARGS rms, mode, x, res, res_bias, sum_out, w, b, y, mean, rstd, rows, N, eps, key, (uint32_t)thr, scale, st
  if (xdt == kBF16 && wdt == kBF16) return dispatch_site<bf16_t, bf16_t>(PDT_ARGS);
  if (xdt == kBF16 && wdt == kF32) return dispatch_site<bf16_t, float>(PDT_ARGS);
  if (xdt == kF32 && wdt == kF32) return dispatch_site<float, float>(PDT_ARGS);
  if (xdt == kF32 && wdt == kBF16) return dispatch_site<float, bf16_t>(PDT_ARGS);
#undef PDT_ARGS
  return (int)hipErrorInvalidValue;
}
