// Multi-tensor optimizer-side kernels for gfx950: fused AdamW, fused SGD, two-stage fused LAMB, fused L2-norm /
// non-finite check, clip-coefficient, and in-place scale.  One launch covers every tensor in a list.
//
// Replaces the per-parameter foreach chain torch runs for the reference's AdamW + clip_grad_norm_
// (reference: Stoke-DDP.py:226-235 AdamW(lr, betas=(0.9,0.99), eps, wd), Stoke-DDP.py:253
// ClipGradNormConfig(max_norm, norm_type=2); Fairscale-DDP.py:78-86) -- the math order follows
// torch/optim/adam.py:419-547 / torch's fused AdamW so checkpoints interoperate.
//
// Tensor lists are described by a device int64 table, 6 words per tensor:
//   [ptr0, ptr1, ptr2, ptr3, ptr4, numel]
// and a block table (int32 pairs: tensor index, chunk index).  The engines keep parameters in flat
// buffers, so the common case is a 1-entry table whose chunks tile the whole shard; the table form
// is what lets a user hand the optimizer arbitrary parameter lists and still get ONE launch.
// The parameter-EMA variants of the step kernels take a second table with the same row order, ONE pointer
// per row (the fp32 average; null = the row keeps none): the 6-word row is full for AdamW and is shared
// with every other kernel here, so it is not widened.
//
// Sync-free step: the grad multiplier (1/loss_scale * clip coefficient) and the found_inf flag live in
// device memory, produced by pdt_l2norm_* + pdt_clip_coef, so no host round trip sits between
// backward and the optimizer.
#include "common.h"

using namespace pdt;

namespace {

constexpr int MT_META = 6;
constexpr int MT_THREADS = 256;

struct AdamHyper {
  float lr, beta1, beta2, eps, wd;
  float step_size;  // lr / (1 - beta1^t)
  float bc2_sqrt;   // sqrt(1 - beta2^t)
  int decoupled;    // 1 = AdamW, 0 = Adam (L2 added to the gradient)
};

template <typename G>
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float g, const AdamHyper& h) {
  if (h.decoupled) {
    p *= 1.f - h.lr * h.wd;
  } else if (h.wd != 0.f) {
    g += h.wd * p;
  }
  m = h.beta1 * m + (1.f - h.beta1) * g;
  v = h.beta2 * v + (1.f - h.beta2) * g * g;
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  p -= h.step_size * m / denom;
}

// Parameter EMA (torch.optim.swa_utils.get_ema_multi_avg_fn: lerp(ema, p, 1 - decay)): e <- e + w * (p - e) with the
// freshly updated fp32 p still in registers.  The product and the sum may contract into one FMA (one rounding fewer).
__device__ __forceinline__ float ema_elem(float e, float p, float w) { return e + w * (p - e); }

// One block processes one chunk of one tensor; 4 elements per thread per iteration (16-B loads).
// EMA: ``ema_tab[row]`` is the row's fp32 average (null = none), updated from the new p next to the P / M / V / O stores.
template <typename G, bool EMA = false>
__global__ __launch_bounds__(MT_THREADS) void adamw_mt_kernel(
    const int64_t* __restrict__ meta, const int* __restrict__ blk, int chunk, AdamHyper h,
    const float* __restrict__ gscale, const int* __restrict__ found_inf, const float* __restrict__ dstep,
    const int64_t* __restrict__ ema_tab = nullptr, float ema_w = 0.f) {
  if (found_inf != nullptr && *found_inf != 0) return;  // GradScaler semantics: skip the step
  const float gs = gscale ? *gscale : 1.f;
  if (dstep != nullptr) {   // graph-capturable: the step count lives on the device, bias corrections here
    const float t = *dstep;
    h.step_size = h.lr / (1.f - powf(h.beta1, t));
    h.bc2_sqrt = sqrtf(1.f - powf(h.beta2, t));
  }
  const int t = blk[2 * blockIdx.x], c = blk[2 * blockIdx.x + 1];
  const int64_t* mt = meta + (int64_t)t * MT_META;
  float* __restrict__ P = reinterpret_cast<float*>(mt[0]);
  const G* __restrict__ Gr = reinterpret_cast<const G*>(mt[1]);
  float* __restrict__ M = reinterpret_cast<float*>(mt[2]);
  float* __restrict__ V = reinterpret_cast<float*>(mt[3]);
  bf16_t* __restrict__ O = reinterpret_cast<bf16_t*>(mt[4]);
  const int64_t ea = EMA ? ema_tab[t] : 0;
  float* __restrict__ E = reinterpret_cast<float*>(ea);
  const int64_t n = mt[5];
  const int64_t beg = (int64_t)c * chunk;
  const int64_t end = beg + chunk < n ? beg + chunk : n;
  const bool vec_ok = ((mt[0] | mt[1] | mt[2] | mt[3] | ea) & 15) == 0 && (mt[4] & 7) == 0 &&
                      (sizeof(G) == 4 || (mt[1] & 7) == 0);
  int64_t i = beg + (int64_t)threadIdx.x * 4;
  if (vec_ok) {
    for (; i + 3 < end; i += MT_THREADS * 4) {
      f32x4 p = *reinterpret_cast<f32x4*>(P + i);
      f32x4 m = *reinterpret_cast<f32x4*>(M + i);
      f32x4 v = *reinterpret_cast<f32x4*>(V + i);
      float g[4];
      if constexpr (sizeof(G) == 4) {
        f32x4 gg = *reinterpret_cast<const f32x4*>(Gr + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = gg[k];
      } else {
        u16x4 gg = *reinterpret_cast<const u16x4*>(Gr + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = bf2f(gg[k]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = p[k], mk = m[k], vk = v[k];
        adam_elem<G>(pk, mk, vk, g[k] * gs, h);
        p[k] = pk; m[k] = mk; v[k] = vk;
      }
      *reinterpret_cast<f32x4*>(P + i) = p;
      *reinterpret_cast<f32x4*>(M + i) = m;
      *reinterpret_cast<f32x4*>(V + i) = v;
      if (EMA && E) {
        f32x4 e = *reinterpret_cast<f32x4*>(E + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = ema_elem(e[k], p[k], ema_w);
        *reinterpret_cast<f32x4*>(E + i) = e;
      }
      if (O) {
        u16x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = f2bf(p[k]);
        *reinterpret_cast<u16x4*>(O + i) = o;
      }
    }
    // tail (fewer than 4 left for this thread)
    for (; i < end; ++i) {
      float p = P[i], m = M[i], v = V[i];
      adam_elem<G>(p, m, v, to_f<G>(Gr[i]) * gs, h);
      P[i] = p; M[i] = m; V[i] = v;
      if (EMA && E) E[i] = ema_elem(E[i], p, ema_w);
      if (O) O[i] = f2bf(p);
    }
  } else {
    for (int64_t j = beg + threadIdx.x; j < end; j += MT_THREADS) {
      float p = P[j], m = M[j], v = V[j];
      adam_elem<G>(p, m, v, to_f<G>(Gr[j]) * gs, h);
      P[j] = p; M[j] = m; V[j] = v;
      if (EMA && E) E[j] = ema_elem(E[j], p, ema_w);
      if (O) O[j] = f2bf(p);
    }
  }
}

struct SgdHyper {
  float lr, momentum, wd;
  int nesterov;
};

// torch/optim/sgd.py _single_tensor_sgd with dampening 0: a zero-initialised buffer reproduces torch's first
// step (buf = clone(g) == momentum * 0 + g), so there is no step count and a skipped step is exact.
template <bool MOM>
__device__ __forceinline__ void sgd_elem(float& p, float& b, float g, const SgdHyper& h) {
  if (h.wd != 0.f) g += h.wd * p;
  if (MOM) {
    b = h.momentum * b + g;
    g = h.nesterov ? g + h.momentum * b : b;
  }
  p -= h.lr * g;
}

// Same table / block form as adamw_mt_kernel: [param f32, grad, momentum_buffer f32 or null, unused, bf16 out or
// null, numel].  A null buffer column (momentum == 0) is neither read nor written.  E: the row's fp32 parameter
// average (EMA instantiations only; null = none).
template <typename G, bool MOM, bool EMA>
__device__ __forceinline__ void sgd_chunk(const int64_t* __restrict__ mt, int c, int chunk, const SgdHyper& h,
                                          float gs, float* __restrict__ E, float ema_w) {
  float* __restrict__ P = reinterpret_cast<float*>(mt[0]);
  const G* __restrict__ Gr = reinterpret_cast<const G*>(mt[1]);
  float* __restrict__ M = reinterpret_cast<float*>(mt[2]);
  bf16_t* __restrict__ O = reinterpret_cast<bf16_t*>(mt[4]);
  const int64_t n = mt[5];
  const int64_t beg = (int64_t)c * chunk;
  const int64_t end = beg + chunk < n ? beg + chunk : n;
  const bool vec_ok = ((mt[0] | mt[1] | mt[2] | (EMA ? reinterpret_cast<int64_t>(E) : 0)) & 15) == 0 &&
                      (mt[4] & 7) == 0 && (sizeof(G) == 4 || (mt[1] & 7) == 0);
  int64_t i = beg + (int64_t)threadIdx.x * 4;
  if (vec_ok) {
    for (; i + 3 < end; i += MT_THREADS * 4) {
      f32x4 p = *reinterpret_cast<f32x4*>(P + i);
      f32x4 m = {0.f, 0.f, 0.f, 0.f};
      if (MOM) m = *reinterpret_cast<f32x4*>(M + i);
      float g[4];
      if constexpr (sizeof(G) == 4) {
        f32x4 gg = *reinterpret_cast<const f32x4*>(Gr + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = gg[k];
      } else {
        u16x4 gg = *reinterpret_cast<const u16x4*>(Gr + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = bf2f(gg[k]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = p[k], mk = m[k];
        sgd_elem<MOM>(pk, mk, g[k] * gs, h);
        p[k] = pk; m[k] = mk;
      }
      *reinterpret_cast<f32x4*>(P + i) = p;
      if (MOM) *reinterpret_cast<f32x4*>(M + i) = m;
      if (EMA && E) {
        f32x4 e = *reinterpret_cast<f32x4*>(E + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = ema_elem(e[k], p[k], ema_w);
        *reinterpret_cast<f32x4*>(E + i) = e;
      }
      if (O) {
        u16x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = f2bf(p[k]);
        *reinterpret_cast<u16x4*>(O + i) = o;
      }
    }
    // tail (fewer than 4 left for this thread)
    for (; i < end; ++i) {
      float p = P[i], m = MOM ? M[i] : 0.f;
      sgd_elem<MOM>(p, m, to_f<G>(Gr[i]) * gs, h);
      P[i] = p;
      if (MOM) M[i] = m;
      if (EMA && E) E[i] = ema_elem(E[i], p, ema_w);
      if (O) O[i] = f2bf(p);
    }
  } else {
    for (int64_t j = beg + threadIdx.x; j < end; j += MT_THREADS) {
      float p = P[j], m = MOM ? M[j] : 0.f;
      sgd_elem<MOM>(p, m, to_f<G>(Gr[j]) * gs, h);
      P[j] = p;
      if (MOM) M[j] = m;
      if (EMA && E) E[j] = ema_elem(E[j], p, ema_w);
      if (O) O[j] = f2bf(p);
    }
  }
}

// Fused SGD (momentum / Nesterov, L2 weight decay).  lr_ptr: the learning rate read from the device, so a
// captured step follows a schedule that fills the tensor in place.
template <typename G, bool EMA = false>
__global__ __launch_bounds__(MT_THREADS) void sgd_mt_kernel(
    const int64_t* __restrict__ meta, const int* __restrict__ blk, int chunk, SgdHyper h,
    const float* __restrict__ gscale, const int* __restrict__ found_inf, const float* __restrict__ lr_ptr,
    const int64_t* __restrict__ ema_tab = nullptr, float ema_w = 0.f) {
  if (found_inf != nullptr && *found_inf != 0) return;  // GradScaler semantics: skip the step
  const float gs = gscale ? *gscale : 1.f;
  if (lr_ptr != nullptr) h.lr = *lr_ptr;
  const int t = blk[2 * blockIdx.x], c = blk[2 * blockIdx.x + 1];
  const int64_t* mt = meta + (int64_t)t * MT_META;
  float* E = EMA ? reinterpret_cast<float*>(ema_tab[t]) : nullptr;
  if (h.momentum != 0.f && mt[2] != 0)
    sgd_chunk<G, true, EMA>(mt, c, chunk, h, gs, E, ema_w);
  else
    sgd_chunk<G, false, EMA>(mt, c, chunk, h, gs, E, ema_w);
}

// ---- LAMB (You et al., "Large Batch Optimization for Deep Learning"; apex FusedLAMB / timm Lamb without the clip).
// Per logical tensor:  u = m_hat / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd * p,  r = ||p|| / ||u||,  p -= lr * r * u.
// The ratio needs the norms of the WHOLE tensor before any element moves, so the step is two passes over the 6-word
// table with a tiny per-row reduction between them (and, where a tensor is cut by a rank boundary, the caller's
// all-reduce of ``sums``).  Stage 2 recomputes u from (p, m, v) instead of reading a stored copy: the same bytes,
// no [numel] fp32 scratch.
struct LambHyper {
  float lr, beta1, beta2, eps, wd;
  float omb1, omb2;  // 1 - beta1, 1 - beta2 rounded from double: 1.f - 0.999f is 6e-5 (relative) off 0.001
  float bc1;       // 1 - beta1^t
  float bc2_sqrt;  // sqrt(1 - beta2^t)
  int adapt;       // 0: r = 1 (wd == 0 without always_adapt: bias-corrected Adam)
};

// the per-row int table that goes with the block table: [first block, number of blocks, logical-tensor index]
constexpr int LAMB_ROW = 3;

__device__ __forceinline__ void lamb_bias(LambHyper& h, const float* __restrict__ dstep) {
  if (dstep != nullptr) {   // graph-capturable: the step count lives on the device, bias corrections here
    // 1 - beta^t = -expm1(t log1p(-(1 - beta))): exact to rounding where beta^t is close to 1
    const float t = *dstep;
    h.bc1 = -expm1f(t * log1pf(-h.omb1));
    h.bc2_sqrt = sqrtf(-expm1f(t * log1pf(-h.omb2)));
  }
}

__device__ __forceinline__ void lamb_moments(float& m, float& v, float g, const LambHyper& h) {
  m = h.beta1 * m + h.omb1 * g;
  v = h.beta2 * v + h.omb2 * g * g;
}

// The update direction from the NEW moments and the OLD parameter: the ONE function both stages call.  The compiler
// may still contract it differently at its two inline sites, so stage 2's u need not be the bit pattern stage 1
// summed; that is accepted -- the sums only enter through the ratio of two norms.
__device__ __forceinline__ float lamb_update(float p, float m, float v, const LambHyper& h) {
  return (m / h.bc1) / (sqrtf(v) / h.bc2_sqrt + h.eps) + h.wd * p;
}

// Stage 1: new moments stored, u formed in registers, partial[2 * block] = (sum p*p, sum u*u) over the block's chunk.
template <typename G>
__global__ __launch_bounds__(MT_THREADS) void lamb_stage1_mt_kernel(
    const int64_t* __restrict__ meta, const int* __restrict__ blk, int chunk, LambHyper h,
    const float* __restrict__ gscale, const int* __restrict__ found_inf, const float* __restrict__ dstep,
    float* __restrict__ partial) {
  __shared__ float red[MT_THREADS / 64];
  if (found_inf != nullptr && *found_inf != 0) return;  // GradScaler semantics: skip the step
  const float gs = gscale ? *gscale : 1.f;
  lamb_bias(h, dstep);
  const int t = blk[2 * blockIdx.x], c = blk[2 * blockIdx.x + 1];
  const int64_t* mt = meta + (int64_t)t * MT_META;
  const float* __restrict__ P = reinterpret_cast<const float*>(mt[0]);
  const G* __restrict__ Gr = reinterpret_cast<const G*>(mt[1]);
  float* __restrict__ M = reinterpret_cast<float*>(mt[2]);
  float* __restrict__ V = reinterpret_cast<float*>(mt[3]);
  const int64_t n = mt[5];
  const int64_t beg = (int64_t)c * chunk;
  const int64_t end = beg + chunk < n ? beg + chunk : n;
  const bool vec_ok = ((mt[0] | mt[1] | mt[2] | mt[3]) & 15) == 0 && (sizeof(G) == 4 || (mt[1] & 7) == 0);
  float pp = 0.f, uu = 0.f;
  int64_t i = beg + (int64_t)threadIdx.x * 4;
  if (vec_ok) {
    for (; i + 3 < end; i += MT_THREADS * 4) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(P + i);
      f32x4 m = *reinterpret_cast<f32x4*>(M + i);
      f32x4 v = *reinterpret_cast<f32x4*>(V + i);
      float g[4];
      if constexpr (sizeof(G) == 4) {
        f32x4 gg = *reinterpret_cast<const f32x4*>(Gr + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = gg[k];
      } else {
        u16x4 gg = *reinterpret_cast<const u16x4*>(Gr + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = bf2f(gg[k]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float mk = m[k], vk = v[k];
        lamb_moments(mk, vk, g[k] * gs, h);
        const float u = lamb_update(p[k], mk, vk, h);
        pp += p[k] * p[k];
        uu += u * u;
        m[k] = mk; v[k] = vk;
      }
      *reinterpret_cast<f32x4*>(M + i) = m;
      *reinterpret_cast<f32x4*>(V + i) = v;
    }
    // tail (fewer than 4 left for this thread)
    for (; i < end; ++i) {
      const float p = P[i];
      float m = M[i], v = V[i];
      lamb_moments(m, v, to_f<G>(Gr[i]) * gs, h);
      const float u = lamb_update(p, m, v, h);
      pp += p * p;
      uu += u * u;
      M[i] = m; V[i] = v;
    }
  } else {
    for (int64_t j = beg + threadIdx.x; j < end; j += MT_THREADS) {
      const float p = P[j];
      float m = M[j], v = V[j];
      lamb_moments(m, v, to_f<G>(Gr[j]) * gs, h);
      const float u = lamb_update(p, m, v, h);
      pp += p * p;
      uu += u * u;
      M[j] = m; V[j] = v;
    }
  }
  pp = block_sum<MT_THREADS / 64>(pp, red);
  uu = block_sum<MT_THREADS / 64>(uu, red);
  if (threadIdx.x == 0) {
    partial[2 * (int64_t)blockIdx.x] = pp;
    partial[2 * (int64_t)blockIdx.x + 1] = uu;
  }
}

// One workgroup per row: the row's blocks are consecutive in the block table, so its partials are
// partial[2 * first .. 2 * (first + count)).  Fixed order and no float atomics: bitwise reproducible.  sums is
// zero-filled by the caller and a logical tensor sits on at most one row of a step, so a plain store is enough and a
// rank holding no part of a tensor contributes 0 to the all-reduce.
__global__ __launch_bounds__(MT_THREADS) void lamb_rowsum_kernel(const float* __restrict__ partial,
                                                                 const int* __restrict__ rows,
                                                                 const int* __restrict__ found_inf,
                                                                 float* __restrict__ sums) {
  __shared__ float red[MT_THREADS / 64];
  if (found_inf != nullptr && *found_inf != 0) return;  // stage 1 wrote no partials
  const int* r = rows + LAMB_ROW * (int64_t)blockIdx.x;
  const int first = r[0], count = r[1], gid = r[2];
  float pp = 0.f, uu = 0.f;
  for (int b = threadIdx.x; b < count; b += MT_THREADS) {
    pp += partial[2 * (int64_t)(first + b)];
    uu += partial[2 * (int64_t)(first + b) + 1];
  }
  pp = block_sum<MT_THREADS / 64>(pp, red);
  uu = block_sum<MT_THREADS / 64>(uu, red);
  if (threadIdx.x == 0) {
    sums[2 * (int64_t)gid] = pp;
    sums[2 * (int64_t)gid + 1] = uu;
  }
}

// Stage 2: r from the row's (all-reduced) sums, u recomputed through lamb_update, p / bf16 copy / EMA stored.
template <bool EMA>
__global__ __launch_bounds__(MT_THREADS) void lamb_stage2_mt_kernel(
    const int64_t* __restrict__ meta, const int* __restrict__ blk, int chunk, LambHyper h,
    const int* __restrict__ found_inf, const float* __restrict__ dstep, const int* __restrict__ rows,
    const float* __restrict__ sums, const int64_t* __restrict__ ema_tab, float ema_w) {
  if (found_inf != nullptr && *found_inf != 0) return;  // GradScaler semantics: skip the step
  lamb_bias(h, dstep);
  const int t = blk[2 * blockIdx.x], c = blk[2 * blockIdx.x + 1];
  const int64_t* mt = meta + (int64_t)t * MT_META;
  float* __restrict__ P = reinterpret_cast<float*>(mt[0]);
  const float* __restrict__ M = reinterpret_cast<const float*>(mt[2]);
  const float* __restrict__ V = reinterpret_cast<const float*>(mt[3]);
  bf16_t* __restrict__ O = reinterpret_cast<bf16_t*>(mt[4]);
  const int64_t ea = EMA ? ema_tab[t] : 0;
  float* __restrict__ E = reinterpret_cast<float*>(ea);
  const int gid = rows[LAMB_ROW * (int64_t)t + 2];
  const float pn = sums[2 * (int64_t)gid], un = sums[2 * (int64_t)gid + 1];
  const float ratio = (h.adapt && pn > 0.f && un > 0.f) ? sqrtf(pn) / sqrtf(un) : 1.f;
  const float step = h.lr * ratio;
  const int64_t n = mt[5];
  const int64_t beg = (int64_t)c * chunk;
  const int64_t end = beg + chunk < n ? beg + chunk : n;
  const bool vec_ok = ((mt[0] | mt[2] | mt[3] | ea) & 15) == 0 && (mt[4] & 7) == 0;
  int64_t i = beg + (int64_t)threadIdx.x * 4;
  if (vec_ok) {
    for (; i + 3 < end; i += MT_THREADS * 4) {
      f32x4 p = *reinterpret_cast<f32x4*>(P + i);
      const f32x4 m = *reinterpret_cast<const f32x4*>(M + i);
      const f32x4 v = *reinterpret_cast<const f32x4*>(V + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) p[k] -= step * lamb_update(p[k], m[k], v[k], h);
      *reinterpret_cast<f32x4*>(P + i) = p;
      if (EMA && E) {
        f32x4 e = *reinterpret_cast<f32x4*>(E + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = ema_elem(e[k], p[k], ema_w);
        *reinterpret_cast<f32x4*>(E + i) = e;
      }
      if (O) {
        u16x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = f2bf(p[k]);
        *reinterpret_cast<u16x4*>(O + i) = o;
      }
    }
    // tail (fewer than 4 left for this thread)
    for (; i < end; ++i) {
      float p = P[i];
      p -= step * lamb_update(p, M[i], V[i], h);
      P[i] = p;
      if (EMA && E) E[i] = ema_elem(E[i], p, ema_w);
      if (O) O[i] = f2bf(p);
    }
  } else {
    for (int64_t j = beg + threadIdx.x; j < end; j += MT_THREADS) {
      float p = P[j];
      p -= step * lamb_update(p, M[j], V[j], h);
      P[j] = p;
      if (EMA && E) E[j] = ema_elem(E[j], p, ema_w);
      if (O) O[j] = f2bf(p);
    }
  }
}

// Sum of squares per block (ptr0 of each tensor), written to partial[blockIdx.x].
template <typename G>
__global__ __launch_bounds__(MT_THREADS) void l2norm_mt_kernel(const int64_t* __restrict__ meta,
                                                               const int* __restrict__ blk, int chunk,
                                                               float* __restrict__ partial) {
  __shared__ float red[MT_THREADS / 64];
  const int t = blk[2 * blockIdx.x], c = blk[2 * blockIdx.x + 1];
  const int64_t* mt = meta + (int64_t)t * MT_META;
  const G* __restrict__ X = reinterpret_cast<const G*>(mt[0]);
  const int64_t n = mt[5];
  const int64_t beg = (int64_t)c * chunk;
  const int64_t end = beg + chunk < n ? beg + chunk : n;
  float acc = 0.f;
  const bool vec_ok = (mt[0] & 15) == 0;
  int64_t i = beg + (int64_t)threadIdx.x * 8;
  if (vec_ok) {
    for (; i + 7 < end; i += MT_THREADS * 8) {
      float x[8];
      Vec8<G>::load(X + i, x);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += x[k] * x[k];
    }
    for (; i < end; ++i) { float x = to_f<G>(X[i]); acc += x * x; }
  } else {
    for (int64_t j = beg + threadIdx.x; j < end; j += MT_THREADS) { float x = to_f<G>(X[j]); acc += x * x; }
  }
  acc = block_sum<MT_THREADS / 64>(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// Deterministic final reduction of the per-block partials (fixed order: bitwise reproducible).
__global__ __launch_bounds__(1024) void reduce_partials_kernel(const float* __restrict__ partial, int n,
                                                               float* __restrict__ out, int accumulate) {
  __shared__ float red[16];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) acc += partial[i];
  acc = block_sum<16>(acc, red);
  if (threadIdx.x == 0) out[0] = accumulate ? out[0] + acc : acc;
}

// total_sq holds the (already globally all-reduced) sum of squares of the *scaled* gradients.
// Writes: norm_out = ||g|| / loss_scale, coef_out = grad multiplier = clip_coef / loss_scale,
// found_inf = !isfinite(total).  clip_coef = min(1, max_norm / (norm + 1e-6))
// (torch/nn/utils/clip_grad.py:165-174).  max_norm <= 0 disables clipping.
__global__ void clip_coef_kernel(const float* __restrict__ total_sq, float max_norm, const float* inv_scale_ptr,
                                 float inv_scale_val, float* __restrict__ norm_out, float* __restrict__ coef_out,
                                 int* __restrict__ found_inf) {
  const float inv_scale = inv_scale_ptr ? *inv_scale_ptr : inv_scale_val;
  const float sq = total_sq[0];
  const float norm = sqrtf(sq) * inv_scale;
  const bool finite = isfinite(sq);
  float coef = 1.f;
  if (max_norm > 0.f && finite) coef = fminf(max_norm / (norm + 1e-6f), 1.f);
  if (norm_out) norm_out[0] = norm;
  if (coef_out) coef_out[0] = coef * inv_scale;
  if (found_inf) found_inf[0] = finite ? 0 : 1;
}

template <typename G>
__global__ __launch_bounds__(MT_THREADS) void scale_mt_kernel(const int64_t* __restrict__ meta,
                                                              const int* __restrict__ blk, int chunk,
                                                              const float* __restrict__ s_ptr) {
  const float s = *s_ptr;
  const int t = blk[2 * blockIdx.x], c = blk[2 * blockIdx.x + 1];
  const int64_t* mt = meta + (int64_t)t * MT_META;
  G* __restrict__ X = reinterpret_cast<G*>(mt[0]);
  const int64_t n = mt[5];
  const int64_t beg = (int64_t)c * chunk;
  const int64_t end = beg + chunk < n ? beg + chunk : n;
  for (int64_t j = beg + threadIdx.x; j < end; j += MT_THREADS) X[j] = from_f<G>(to_f<G>(X[j]) * s);
}

// fp32 -> bf16 copy over a tensor list (ptr0 = src fp32, ptr1 = dst bf16): used to refresh the
// low-precision compute copy of parameters outside the optimizer (e.g. after load_state_dict).
__global__ __launch_bounds__(MT_THREADS) void cast_f32_bf16_mt_kernel(const int64_t* __restrict__ meta,
                                                                      const int* __restrict__ blk, int chunk) {
  const int t = blk[2 * blockIdx.x], c = blk[2 * blockIdx.x + 1];
  const int64_t* mt = meta + (int64_t)t * MT_META;
  const float* __restrict__ S = reinterpret_cast<const float*>(mt[0]);
  bf16_t* __restrict__ D = reinterpret_cast<bf16_t*>(mt[1]);
  const int64_t n = mt[5];
  const int64_t beg = (int64_t)c * chunk;
  const int64_t end = beg + chunk < n ? beg + chunk : n;
  for (int64_t j = beg + threadIdx.x; j < end; j += MT_THREADS) D[j] = f2bf(S[j]);
}

// dst <- src over a tensor list (ptr0 = dst, ptr1 = src, same element type; src 0 -> dst zero-filled): gathers
// per-parameter gradients into a flat buffer in ONE launch (parallel/ddp.py, single-process compute-copy mode)
template <typename T>
__global__ __launch_bounds__(MT_THREADS) void copy_mt_kernel(const int64_t* __restrict__ meta, const int* __restrict__ blk,
                                                             int chunk) {
  const int t = blk[2 * blockIdx.x], c = blk[2 * blockIdx.x + 1];
  const int64_t* mt = meta + (int64_t)t * MT_META;
  T* __restrict__ D = reinterpret_cast<T*>(mt[0]);
  const T* __restrict__ S = reinterpret_cast<const T*>(mt[1]);
  const int64_t n = mt[5];
  const int64_t beg = (int64_t)c * chunk;
  const int64_t end = beg + chunk < n ? beg + chunk : n;
  for (int64_t j = beg + threadIdx.x; j < end; j += MT_THREADS) D[j] = S ? S[j] : T(0);
}

// dst += src for every (dst, src) pair of the table (fp32 arithmetic; a null src adds nothing) -- per-parameter
// gradients accumulated into a flat buffer in ONE launch (DDP gradient stealing across accumulation micro-steps)
template <typename T>
__global__ __launch_bounds__(MT_THREADS) void add_mt_kernel(const int64_t* __restrict__ meta, const int* __restrict__ blk,
                                                            int chunk) {
  const int t = blk[2 * blockIdx.x], c = blk[2 * blockIdx.x + 1];
  const int64_t* mt = meta + (int64_t)t * MT_META;
  T* __restrict__ D = reinterpret_cast<T*>(mt[0]);
  const T* __restrict__ S = reinterpret_cast<const T*>(mt[1]);
  if (S == nullptr) return;
  const int64_t n = mt[5];
  const int64_t beg = (int64_t)c * chunk;
  const int64_t end = beg + chunk < n ? beg + chunk : n;
  for (int64_t j = beg + threadIdx.x; j < end; j += MT_THREADS) D[j] = from_f<T>(to_f<T>(D[j]) + to_f<T>(S[j]));
}

// a <-> b over a tensor list (ptr0 = a fp32, ptr1 = b fp32, ptr2 = bf16 copy of the NEW a or null) in one pass:
// puts the averaged weights (b = the EMA state) into the masters and refreshes the bf16 compute copy with the
// optimizer epilogue's rounding; the same launch again undoes it exactly.
__global__ __launch_bounds__(MT_THREADS) void swap_mt_kernel(const int64_t* __restrict__ meta,
                                                             const int* __restrict__ blk, int chunk) {
  const int t = blk[2 * blockIdx.x], c = blk[2 * blockIdx.x + 1];
  const int64_t* mt = meta + (int64_t)t * MT_META;
  float* __restrict__ A = reinterpret_cast<float*>(mt[0]);
  float* __restrict__ B = reinterpret_cast<float*>(mt[1]);
  bf16_t* __restrict__ O = reinterpret_cast<bf16_t*>(mt[2]);
  const int64_t n = mt[5];
  const int64_t beg = (int64_t)c * chunk;
  const int64_t end = beg + chunk < n ? beg + chunk : n;
  const bool vec_ok = ((mt[0] | mt[1]) & 15) == 0 && (mt[2] & 7) == 0;
  if (vec_ok) {
    int64_t i = beg + (int64_t)threadIdx.x * 4;
    for (; i + 3 < end; i += MT_THREADS * 4) {
      const f32x4 a = *reinterpret_cast<f32x4*>(A + i);
      const f32x4 b = *reinterpret_cast<f32x4*>(B + i);
      *reinterpret_cast<f32x4*>(A + i) = b;
      *reinterpret_cast<f32x4*>(B + i) = a;
      if (O) {
        u16x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = f2bf(b[k]);
        *reinterpret_cast<u16x4*>(O + i) = o;
      }
    }
    for (; i < end; ++i) {   // tail (fewer than 4 left for this thread)
      const float a = A[i], b = B[i];
      A[i] = b; B[i] = a;
      if (O) O[i] = f2bf(b);
    }
  } else {
    for (int64_t j = beg + threadIdx.x; j < end; j += MT_THREADS) {
      const float a = A[j], b = B[j];
      A[j] = b; B[j] = a;
      if (O) O[j] = f2bf(b);
    }
  }
}

// Device step counter of a param group: +1 unless the (all-reduced) found_inf flag says the step is skipped
// (torch.amp.GradScaler skips optimizer.step() on overflow, so Adam's bias-correction step must not move).
__global__ void step_inc_kernel(float* __restrict__ dstep, const int* __restrict__ found_inf) {
  if (threadIdx.x == 0 && (found_inf == nullptr || *found_inf == 0)) dstep[0] = dstep[0] + 1.f;
}

}  // namespace

PDT_API int pdt_step_inc(float* dstep, const int* found_inf, hipStream_t stream) {
  step_inc_kernel<<<1, 64, 0, stream>>>(dstep, found_inf);
  return (int)hipGetLastError();
}

PDT_API int pdt_adamw_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, int grad_dtype, float lr,
                         float beta1, float beta2, float eps, float wd, float step_size, float bc2_sqrt,
                         int decoupled, const float* gscale, const int* found_inf, const float* dstep,
                         hipStream_t stream) {
  AdamHyper h{lr, beta1, beta2, eps, wd, step_size, bc2_sqrt, decoupled};
  if (nblocks <= 0) return 0;
  if (grad_dtype == kF32)
    adamw_mt_kernel<float><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, h, gscale, found_inf, dstep);
  else
    adamw_mt_kernel<bf16_t><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, h, gscale, found_inf, dstep);
  return (int)hipGetLastError();
}

// pdt_adamw_mt + parameter EMA: ema_tab[row] = the row's fp32 average or null, ema_w = 1 - decay
PDT_API int pdt_adamw_ema_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, int grad_dtype, float lr,
                             float beta1, float beta2, float eps, float wd, float step_size, float bc2_sqrt,
                             int decoupled, const float* gscale, const int* found_inf, const float* dstep,
                             const int64_t* ema_tab, float ema_w, hipStream_t stream) {
  AdamHyper h{lr, beta1, beta2, eps, wd, step_size, bc2_sqrt, decoupled};
  if (nblocks <= 0) return 0;
  if (ema_tab == nullptr) return (int)hipErrorInvalidValue;
  if (grad_dtype == kF32)
    adamw_mt_kernel<float, true><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, h, gscale, found_inf, dstep,
                                                                     ema_tab, ema_w);
  else if (grad_dtype == kBF16)
    adamw_mt_kernel<bf16_t, true><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, h, gscale, found_inf, dstep,
                                                                      ema_tab, ema_w);
  else
    return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

// lr_ptr (device, nullable) overrides lr; a non-zero momentum needs the buffer column of every row set
PDT_API int pdt_sgd_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, int grad_dtype, float lr,
                       float momentum, float wd, int nesterov, const float* gscale, const int* found_inf,
                       const float* lr_ptr, hipStream_t stream) {
  SgdHyper h{lr, momentum, wd, nesterov};
  if (nblocks <= 0) return 0;
  if (grad_dtype == kF32)
    sgd_mt_kernel<float><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, h, gscale, found_inf, lr_ptr);
  else if (grad_dtype == kBF16)
    sgd_mt_kernel<bf16_t><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, h, gscale, found_inf, lr_ptr);
  else
    return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

// pdt_sgd_mt + parameter EMA (as pdt_adamw_ema_mt)
PDT_API int pdt_sgd_ema_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, int grad_dtype, float lr,
                           float momentum, float wd, int nesterov, const float* gscale, const int* found_inf,
                           const float* lr_ptr, const int64_t* ema_tab, float ema_w, hipStream_t stream) {
  SgdHyper h{lr, momentum, wd, nesterov};
  if (nblocks <= 0) return 0;
  if (ema_tab == nullptr) return (int)hipErrorInvalidValue;
  if (grad_dtype == kF32)
    sgd_mt_kernel<float, true><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, h, gscale, found_inf, lr_ptr,
                                                                   ema_tab, ema_w);
  else if (grad_dtype == kBF16)
    sgd_mt_kernel<bf16_t, true><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, h, gscale, found_inf, lr_ptr,
                                                                    ema_tab, ema_w);
  else
    return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

// LAMB stage 1 over rows [param f32, grad, exp_avg f32, exp_avg_sq f32, bf16 out or null, numel]: stores the new
// moments and partial[2 * block] = (sum p*p, sum u*u); partial holds 2 * nblocks floats.  omb = 1 - beta (rounded
// from double by the caller), bc1 = 1 - beta1^t, bc2_sqrt = sqrt(1 - beta2^t); dstep (device, nullable) overrides both.
PDT_API int pdt_lamb_stage1_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, int grad_dtype, float beta1,
                               float beta2, float omb1, float omb2, float eps, float wd, float bc1, float bc2_sqrt,
                               const float* gscale, const int* found_inf, const float* dstep, float* partial,
                               hipStream_t stream) {
  LambHyper h{0.f, beta1, beta2, eps, wd, omb1, omb2, bc1, bc2_sqrt, 0};
  if (nblocks <= 0) return 0;
  if (partial == nullptr) return (int)hipErrorInvalidValue;
  if (grad_dtype == kF32)
    lamb_stage1_mt_kernel<float><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, h, gscale, found_inf, dstep,
                                                                     partial);
  else if (grad_dtype == kBF16)
    lamb_stage1_mt_kernel<bf16_t><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, h, gscale, found_inf, dstep,
                                                                      partial);
  else
    return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

// rows: 3 ints per table row [first block, block count, logical-tensor index]; sums[2 * index] = the row's
// (sum p*p, sum u*u).  sums is zero-filled by the caller; an index sits on at most one row.
PDT_API int pdt_lamb_rowsum(const float* partial, const int* rows, int nrows, const int* found_inf, float* sums,
                            hipStream_t stream) {
  if (nrows <= 0) return 0;
  if (partial == nullptr || rows == nullptr || sums == nullptr) return (int)hipErrorInvalidValue;
  lamb_rowsum_kernel<<<nrows, MT_THREADS, 0, stream>>>(partial, rows, found_inf, sums);
  return (int)hipGetLastError();
}

// LAMB stage 2: p -= lr * r * u with r from sums (after the caller's all-reduce), adapt = 0 forces r = 1
PDT_API int pdt_lamb_stage2_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, float lr, float beta1,
                               float beta2, float omb1, float omb2, float eps, float wd, float bc1, float bc2_sqrt,
                               int adapt, const int* found_inf, const float* dstep, const int* rows,
                               const float* sums, hipStream_t stream) {
  LambHyper h{lr, beta1, beta2, eps, wd, omb1, omb2, bc1, bc2_sqrt, adapt};
  if (nblocks <= 0) return 0;
  if (rows == nullptr || sums == nullptr) return (int)hipErrorInvalidValue;
  lamb_stage2_mt_kernel<false><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, h, found_inf, dstep, rows, sums,
                                                                   nullptr, 0.f);
  return (int)hipGetLastError();
}

// pdt_lamb_stage2_mt + parameter EMA (as pdt_adamw_ema_mt)
PDT_API int pdt_lamb_stage2_ema_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, float lr, float beta1,
                                   float beta2, float omb1, float omb2, float eps, float wd, float bc1,
                                   float bc2_sqrt, int adapt, const int* found_inf, const float* dstep,
                                   const int* rows, const float* sums, const int64_t* ema_tab, float ema_w,
                                   hipStream_t stream) {
  LambHyper h{lr, beta1, beta2, eps, wd, omb1, omb2, bc1, bc2_sqrt, adapt};
  if (nblocks <= 0) return 0;
  if (rows == nullptr || sums == nullptr || ema_tab == nullptr) return (int)hipErrorInvalidValue;
  lamb_stage2_mt_kernel<true><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, h, found_inf, dstep, rows, sums,
                                                                  ema_tab, ema_w);
  return (int)hipGetLastError();
}

// rows [a fp32, b fp32, bf16 out or null, -, -, numel]: a <-> b, out = bf16(new a)
PDT_API int pdt_swap_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, hipStream_t stream) {
  if (nblocks <= 0) return 0;
  swap_mt_kernel<<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk);
  return (int)hipGetLastError();
}

// partial must hold nblocks floats.  out[0] = sum of squares (accumulate=1 adds to out[0]).
PDT_API int pdt_l2norm_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, int dtype, float* partial,
                          float* out, int accumulate, hipStream_t stream) {
  if (nblocks <= 0) {
    if (!accumulate) return (int)hipMemsetAsync(out, 0, sizeof(float), stream);
    return 0;
  }
  if (dtype == kF32)
    l2norm_mt_kernel<float><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, partial);
  else
    l2norm_mt_kernel<bf16_t><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, partial);
  reduce_partials_kernel<<<1, 1024, 0, stream>>>(partial, nblocks, out, accumulate);
  return (int)hipGetLastError();
}

PDT_API int pdt_clip_coef(const float* total_sq, float max_norm, const float* inv_scale_ptr, float inv_scale_val,
                          float* norm_out, float* coef_out, int* found_inf, hipStream_t stream) {
  clip_coef_kernel<<<1, 1, 0, stream>>>(total_sq, max_norm, inv_scale_ptr, inv_scale_val, norm_out, coef_out,
                                        found_inf);
  return (int)hipGetLastError();
}

PDT_API int pdt_scale_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, int dtype, const float* s,
                         hipStream_t stream) {
  if (nblocks <= 0) return 0;
  if (dtype == kF32)
    scale_mt_kernel<float><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, s);
  else
    scale_mt_kernel<bf16_t><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk, s);
  return (int)hipGetLastError();
}

PDT_API int pdt_cast_f32_bf16_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, hipStream_t stream) {
  if (nblocks <= 0) return 0;
  cast_f32_bf16_mt_kernel<<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk);
  return (int)hipGetLastError();
}

// dt: kBF16 or kF32
PDT_API int pdt_add_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, int dt, hipStream_t stream) {
  if (nblocks <= 0) return 0;
  if (dt == kF32)
    add_mt_kernel<float><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk);
  else if (dt == kBF16)
    add_mt_kernel<bf16_t><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk);
  else
    return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

// elem_bytes 2 (bf16 / fp16) or 4 (fp32)
PDT_API int pdt_copy_mt(const int64_t* meta, const int* blk, int nblocks, int chunk, int elem_bytes, hipStream_t stream) {
  if (nblocks <= 0) return 0;
  if (elem_bytes == 4)
    copy_mt_kernel<uint32_t><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk);
  else if (elem_bytes == 2)
    copy_mt_kernel<uint16_t><<<nblocks, MT_THREADS, 0, stream>>>(meta, blk, chunk);
  else
    return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}
