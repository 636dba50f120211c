// Gradient clipping for the optimizers (optimizer.Momentum / SGD / Adam with grad_clip=ClipGradByGlobalNorm / ClipGradByValue,
// Momentum with use_nesterov=True; tests/clip_reference.py is the statement).  All gradients live in one flat arena, so the
// global L2 norm is one streaming reduction over it whose result STAYS on the device: the update kernel reads the clip
// coefficient from a device record.  Nothing here synchronises, downloads or uses an atomic.
//
//   coef    chunk pass: one WAVEFRONT per chunk of kChunk = 4096 gradients, the mapping of msk_intensity_stats (msk_intensity.hip).
//           The statement's lane l of 256 adds g[l]^2, g[l+256]^2, ... in float64; thread m of 64 carries the four lanes
//           4m .. 4m+3: its 16 loads are the quads 64j + m, j = 0..15, so every load instruction of the wavefront is 1 KiB of
//           consecutive bytes and all 16 are issued before the first add.  The tree v[l] += v[l+s] is a xor butterfly over m
//           for s = 128 .. 4 (a + b == b + a bit for bit) and two additions inside the thread for s = 2, 1.  (double)g *
//           (double)g is exact (48 bits of product), so a fused multiply-add gives the same sum as a multiply and an add.
//           The chunk values go to the workspace (8 bytes per 16 KiB of gradient); the finish pass -- one workgroup of 256 --
//           reduces them by the same scheme and one thread writes the record {S, norm, coef, 0}: sqrt and the division are
//           IEEE float64 operations.
//   update  sgd_momentum_k's / adam_k's arithmetic per element (msk_loss_optim.hip) with gs_eff = grad_scale * coef in place
//           of grad_scale; every thread reads the record once, behind its first loads.  Nesterov and the value clamp are
//           template parameters, so the form without them runs the plain kernel's instructions on every element: with
//           coef == 1 its results are bitwise those of msk_sgd_momentum / msk_adam.
#include <cmath>

#include "msk_common.h"

namespace {

constexpr int kChunk = 4096;     // gradients per chunk of the norm
constexpr int kLanes = 256;      // lanes of the statement
constexpr int kThreads = 256;

inline long chunks_of(size_t n) { return (long)((n + kChunk - 1) / kChunk); }

__device__ __forceinline__ double shfl_xor_d(double v, int mask) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_xor(lo, mask, 64);
  hi = __shfl_xor(hi, mask, 64);
  return __hiloint2double(hi, lo);
}

// grid: one wavefront (64 threads) per chunk; g is 16-byte aligned
__global__ void __launch_bounds__(64)
clip_chunk_k(const float* __restrict__ g, long n, double* __restrict__ psq) {
  const int m = threadIdx.x;
  const long base = (long)blockIdx.x * kChunk;
  const long left = n - base;                       // >= 1
  double q[4] = {0.0, 0.0, 0.0, 0.0};
  if (left >= kChunk) {
    const float4* g4 = reinterpret_cast<const float4*>(g + base);
    float4 v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = g4[64 * j + m];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double d = (double)e[i];
        q[i] = q[i] + d * d;
      }
    }
  } else {
    const float* gc = g + base;
    for (int j = 0; j < 16; ++j) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long e = 256L * j + 4 * m + i;
        double d = 0.0;                             // elements past n add the statement's + 0.0
        if (e < left) d = (double)gc[e];
        q[i] = q[i] + d * d;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                // s = 128 .. 4 of the tree
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = q[i] + shfl_xor_d(q[i], o);
  }
  if (m == 0) psq[blockIdx.x] = (q[0] + q[2]) + (q[1] + q[3]);   // s = 2, then s = 1
}

// one workgroup of 256: lane l adds P[l], P[l+256], ... in ascending order, then the tree; thread 0 writes the record
__global__ void __launch_bounds__(kLanes)
clip_finish_k(long nc, const double* __restrict__ psq, float grad_scale, float clip_norm, double* __restrict__ rec) {
  __shared__ double tq[kLanes];
  const int l = threadIdx.x;
  double q = 0.0;
  long c = l;
  for (; c + 7L * kLanes < nc; c += 8L * kLanes) {   // eight loads in flight, added in order
    double b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) b[u] = psq[c + (long)u * kLanes];
#pragma unroll
    for (int u = 0; u < 8; ++u) q = q + b[u];
  }
  for (; c < nc; c += kLanes) q = q + psq[c];
  tq[l] = q;
  __syncthreads();
  for (int o = kLanes / 2; o > 0; o >>= 1) {
    if (l < o) tq[l] = tq[l] + tq[l + o];
    __syncthreads();
  }
  if (l == 0) {
    const double S = tq[0];
    const double cn = (double)clip_norm;
    const double norm = (double)grad_scale * sqrt(S);
    // cn / (norm > cn ? norm : cn) for a finite cn; an infinite cn measures only.  A NaN norm compares false: coef 1
    const float coef = norm > cn ? (float)(cn / norm) : 1.0f;
    rec[0] = S;
    rec[1] = norm;
    rec[2] = (double)coef;
    rec[3] = 0.0;
  }
}

// grad_scale * coef: one float32 product; the record holds coef as a double that is a float32 value
__device__ __forceinline__ float clip_scale(float gs, const double* __restrict__ rec) {
  const float coef = rec != nullptr ? (float)rec[2] : 1.0f;
  return gs * coef;
}

// a NaN gradient stays NaN (the statement's np.minimum / np.maximum propagate it; fmaxf would return the bound)
__device__ __forceinline__ float clamp_value(float g, float lo, float hi) {
  return g != g ? g : fminf(fmaxf(g, lo), hi);
}

template <bool NESTEROV, bool CLAMP>
__device__ __forceinline__ void sgd_one(float& p, float g, float& v, float lr, float mu, float wd, float gs, float lo, float hi) {
  float gg = g * gs;
  if (CLAMP) gg = clamp_value(gg, lo, hi);
  const float t = fmaf(wd, p, gg);
  v = fmaf(mu, v, t);
  if (NESTEROV) {
    const float u = fmaf(mu, v, t);
    p = fmaf(-lr, u, p);
  } else {
    p = fmaf(-lr, v, p);
  }
}

// The first quad's loads are issued BEFORE the record is read: the record is one uniform (scalar) load whose wait would otherwise
// stand, with a second memory latency, in front of every wavefront's first vector load (measured: + 3 us on the 45.6 M arena).
template <bool NESTEROV, bool CLAMP>
__global__ void __launch_bounds__(kThreads)
sgd_momentum_clip_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ vel, size_t n4, size_t n, float lr,
                    float mu, float wd, float gs0, const double* __restrict__ rec, float lo, float hi) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  float4 pp = make_float4(0.f, 0.f, 0.f, 0.f), gg = pp, vv = pp;
  bool more = i < n4;
  if (more) {
    pp = reinterpret_cast<float4*>(p)[i];
    gg = reinterpret_cast<const float4*>(g)[i];
    vv = reinterpret_cast<float4*>(vel)[i];
  }
  __builtin_amdgcn_sched_barrier(0);
  const float gs = clip_scale(gs0, rec);
  while (more) {
    sgd_one<NESTEROV, CLAMP>(pp.x, gg.x, vv.x, lr, mu, wd, gs, lo, hi);
    sgd_one<NESTEROV, CLAMP>(pp.y, gg.y, vv.y, lr, mu, wd, gs, lo, hi);
    sgd_one<NESTEROV, CLAMP>(pp.z, gg.z, vv.z, lr, mu, wd, gs, lo, hi);
    sgd_one<NESTEROV, CLAMP>(pp.w, gg.w, vv.w, lr, mu, wd, gs, lo, hi);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(vel)[i] = vv;
    i += stride;
    more = i < n4;
    if (more) {
      pp = reinterpret_cast<float4*>(p)[i];
      gg = reinterpret_cast<const float4*>(g)[i];
      vv = reinterpret_cast<float4*>(vel)[i];
    }
  }
  // tail
  for (size_t j = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    float ps = p[j], vs = vel[j];
    sgd_one<NESTEROV, CLAMP>(ps, g[j], vs, lr, mu, wd, gs, lo, hi);
    vel[j] = vs;
    p[j] = ps;
  }
}

// adam_k (msk_loss_optim.hip) with the clipped gradient; the expressions are that kernel's, token for token
template <bool CLAMP>
__global__ void __launch_bounds__(kThreads)
adam_clip_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m1, float* __restrict__ m2, size_t n,
            float lr_t, float b1, float b2, float eps_t, float wd, float gs0, const double* __restrict__ rec, float lo, float hi) {
  const float gs = clip_scale(gs0, rec);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float pp = p[i];
    float gc = g[i] * gs;
    if (CLAMP) gc = clamp_value(gc, lo, hi);
    const float gg = fmaf(wd, pp, gc);
    const float a = fmaf(b1, m1[i], (1.f - b1) * gg);
    const float b = fmaf(b2, m2[i], (1.f - b2) * gg * gg);
    m1[i] = a;
    m2[i] = b;
    p[i] = pp - lr_t * (a / (sqrtf(b) + eps_t));
  }
}

inline bool clamp_wanted(float lo, float hi) { return !(lo == -INFINITY && hi == INFINITY); }

}  // namespace

extern "C" {

int msk_grad_clip_workspace(size_t count, size_t* bytes) {
  MSK_REQUIRE(nullptr, bytes != nullptr, "bytes must not be null");
  MSK_REQUIRE(nullptr, count >= 1 && count <= (size_t)0x7fffffff, "count must be in [1, 2^31)");
  *bytes = (size_t)chunks_of(count) * 8;
  return 0;
}

int msk_grad_clip_coef(msk_ctx* ctx, const float* grad, size_t count, float grad_scale, float clip_norm, void* workspace,
                       double* rec) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, grad != nullptr && workspace != nullptr && rec != nullptr, "null grad / workspace / rec");
  MSK_REQUIRE(ctx, count >= 1 && count <= (size_t)0x7fffffff, "count must be in [1, 2^31)");
  MSK_REQUIRE(ctx, clip_norm > 0.f, "clip_norm must be > 0 (+inf measures only)");   // a NaN compares false
  MSK_REQUIRE(ctx, (((uintptr_t)grad) & 15) == 0, "grad must be 16-byte aligned");
  MSK_REQUIRE(ctx, ((((uintptr_t)workspace) | ((uintptr_t)rec)) & 7) == 0, "workspace / rec must be 8-byte aligned");
  if (msk_join_side_impl(ctx) != 0) return -1;   // weight gradients (the late in_tr.conv1 one included) may still be running on the side stream
  const long nc = chunks_of(count);
  double* psq = (double*)workspace;
  {
    msk_launch_scope ls(ctx, "grad_clip_chunks");
    hipLaunchKernelGGL(clip_chunk_k, dim3((unsigned)nc), dim3(64), 0, ctx->stream, grad, (long)count, psq);
  }
  {
    msk_launch_scope ls(ctx, "grad_clip_finish");
    hipLaunchKernelGGL(clip_finish_k, dim3(1), dim3(kLanes), 0, ctx->stream, nc, (const double*)psq, grad_scale, clip_norm, rec);
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

int msk_sgd_momentum_clip(msk_ctx* ctx, float* param, const float* grad, float* velocity, size_t count, float lr, float momentum,
                          float weight_decay, float grad_scale, int nesterov, const double* clip_rec, float clip_min,
                          float clip_max) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  if (count == 0) return 0;
  MSK_REQUIRE(ctx, param != nullptr && grad != nullptr && velocity != nullptr, "null param / grad / velocity");
  MSK_REQUIRE(ctx, ((uintptr_t)param % 16 == 0) && ((uintptr_t)grad % 16 == 0) && ((uintptr_t)velocity % 16 == 0),
              "arenas must be 16-byte aligned");
  MSK_REQUIRE(ctx, (((uintptr_t)clip_rec) & 7) == 0, "clip_rec must be 8-byte aligned");
  MSK_REQUIRE(ctx, !(clip_min > clip_max) && clip_min == clip_min && clip_max == clip_max, "clip_min must be <= clip_max");
  if (msk_join_side_impl(ctx) != 0) return -1;   // weight gradients may still be running on the side stream
  const size_t n4 = count / 4;
  long blocks = (long)((n4 + kThreads - 1) / kThreads);
  const long cap = (long)ctx->num_cu * 16;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  const bool clampv = clamp_wanted(clip_min, clip_max);
  {
    msk_launch_scope ls(ctx, "sgd_momentum_clip");
#define MSK_SGD_CLIP(N_, C_)                                                                                                  \
  hipLaunchKernelGGL((sgd_momentum_clip_k<N_, C_>), dim3((int)blocks), dim3(kThreads), 0, ctx->stream, param, grad, velocity, \
                     n4, count, lr, momentum, weight_decay, grad_scale, clip_rec, clip_min, clip_max)
    if (nesterov) {
      if (clampv) MSK_SGD_CLIP(true, true); else MSK_SGD_CLIP(true, false);
    } else {
      if (clampv) MSK_SGD_CLIP(false, true); else MSK_SGD_CLIP(false, false);
    }
#undef MSK_SGD_CLIP
    MSK_LAUNCH_CHECK(ctx);
  }
  // the packed / transformed forms of the convolution weights inside [param, param + count) are stale now (msk_sgd_momentum)
  msk_weights_changed_impl(ctx, param, count * sizeof(float));
  return msk_wbf_prepack_impl(ctx);
}

int msk_adam_clip(msk_ctx* ctx, float* param, const float* grad, float* moment1, float* moment2, size_t count, float lr,
                  float beta1, float beta2, float epsilon, double beta1_pow, double beta2_pow, float weight_decay,
                  float grad_scale, const double* clip_rec, float clip_min, float clip_max) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  if (count == 0) return 0;
  MSK_REQUIRE(ctx, param != nullptr && grad != nullptr && moment1 != nullptr && moment2 != nullptr, "null param / grad / moments");
  MSK_REQUIRE(ctx, (((uintptr_t)clip_rec) & 7) == 0, "clip_rec must be 8-byte aligned");
  MSK_REQUIRE(ctx, !(clip_min > clip_max) && clip_min == clip_min && clip_max == clip_max, "clip_min must be <= clip_max");
  MSK_REQUIRE(ctx, beta1_pow < 1.0 && beta2_pow < 1.0 && beta1_pow >= 0.0 && beta2_pow >= 0.0, "beta powers must be in [0, 1)");
  if (msk_join_side_impl(ctx) != 0) return -1;   // weight gradients may still be running on the side stream
  const double c2 = sqrt(1.0 - beta2_pow);
  const float lr_t = (float)((double)lr * c2 / (1.0 - beta1_pow));
  const float eps_t = (float)((double)epsilon * c2);
  long blocks = (long)((count + kThreads - 1) / kThreads);
  const long cap = (long)ctx->num_cu * 16;
  if (blocks > cap) blocks = cap;
  {
    msk_launch_scope ls(ctx, "adam_clip");
    if (clamp_wanted(clip_min, clip_max))
      hipLaunchKernelGGL(adam_clip_k<true>, dim3((int)blocks), dim3(kThreads), 0, ctx->stream, param, grad, moment1, moment2, count,
                         lr_t, beta1, beta2, eps_t, weight_decay, grad_scale, clip_rec, clip_min, clip_max);
    else
      hipLaunchKernelGGL(adam_clip_k<false>, dim3((int)blocks), dim3(kThreads), 0, ctx->stream, param, grad, moment1, moment2, count,
                         lr_t, beta1, beta2, eps_t, weight_decay, grad_scale, clip_rec, clip_min, clip_max);
    MSK_LAUNCH_CHECK(ctx);
  }
  msk_weights_changed_impl(ctx, param, count * sizeof(float));
  return msk_wbf_prepack_impl(ctx);
}

}  // extern "C"
