// BCELoss: binary cross entropy with logits, masked by ignore_index (reference losses/binary_cross_entropy_loss.py:84-172).
//
// Per element (y = the target, mask = label != ignore_index, one value per voxel):
//   l = w [ (1 - y) x + (1 + (pw - 1) y) sp(-x) ],  sp(t) = log(1 + e^t)
// The weights are global: w = w_neg + (w_pos - w_neg) y with w_pos / w_neg from the pos / neg counts of the whole target
// ('dynamic') or 1, and pw a constant.  Writing P = (1 - y) sp(x) (= (1 - y)(x + sp(-x))) and Q = y sp(-x):
//   l = w_neg (P + pw Q) + (w_pos - w_neg) (y P + pw y Q)
// so ONE pass over the logits can sum P, Q, yP, yQ and the label counts side by side, and the final kernel applies the
// weights afterwards: no separate labels-only counting pass and no second read of anything.
//
// Thread mapping: a workgroup takes tiles of kTileV voxels.  The tile's labels go through LDS (one coalesced read, the counts
// are taken there), then the workgroup walks the tile's ELEMENTS (voxel-major, class-minor): dense logits (ld == C, 16-byte
// aligned) as float4 quads of consecutive floats, so every access is whole lines whatever C is; a channel slice (ld > C)
// element by element.  An element finds its voxel as i / C through a float reciprocal (exact here, see elem_voxel).
#include "msk_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileV = 1024;     // voxels per tile: 4 labels per thread, <= 64 K elements per tile
constexpr int kNQ = 7;           // partial record: P, Q, yP, yQ (fp32 sums), mask count, pos count, neg count (uint32)

// i / C for 0 <= i < kTileV * 64 (<= 2^16) and 1 <= C <= 64: (i + 0.5) / C lies at least 0.5 / C from an integer, the float
// product's error is below (2^16 / C) * 2^-22 = 2^-6 / C -- truncation gives the exact quotient (C = 1, 2, 4, ...: exact product)
__device__ __forceinline__ int elem_voxel(int i, float inv_c) { return (int)(((float)i + 0.5f) * inv_c); }

// the target of class c at a voxel with label `lab`: C == 1 -> the label value itself; C > 1 -> one_hot(lab, C), all zero for a
// label outside [0, C) (ignore_index included)
__device__ __forceinline__ float bce_target(int lab, int c, int C) { return C == 1 ? (float)lab : (lab == c ? 1.f : 0.f); }

// log(1 + e) for e in [0, 1] from logf of the rounded sum, corrected by e / (u - 1) (u - 1 is exact): a few ulp.  With the
// library's log1pf the forward pass took 0.060 ms at 2 x 128^3, C = 3 (1.1 TB/s); with this, 0.031 ms (both timed back to back,
// logits resident in the last-level cache; from HBM 0.036 ms: profiles/r07_bench_bce.txt)
__device__ __forceinline__ float log1p_unit(float e) {
  const float u = 1.f + e;
  return u == 1.f ? e : logf(u) * __fdividef(e, u - 1.f);
}

struct BceAcc {
  float p = 0.f, q = 0.f, yp = 0.f, yq = 0.f;
  __device__ __forceinline__ void add(float x, int lab, int c, int C, int ignore_index) {
    if (lab == ignore_index) return;
    const float y = bce_target(lab, c, C);
    const float l = log1p_unit(expf(-fabsf(x)));
    const float P = (1.f - y) * (l + fmaxf(x, 0.f));   // (1 - y) sp(x)
    const float Q = y * (l + fmaxf(-x, 0.f));          // y sp(-x)
    p += P;
    q += Q;
    yp = fmaf(y, P, yp);
    yq = fmaf(y, Q, yq);
  }
};

// one pass: labels (counts) + logits (the four sums); partial [nb][kNQ] as 4 floats then 3 uint32 (same 4-byte slots)
__global__ void __launch_bounds__(kThreads)
bce_fwd_k(const float* __restrict__ z, int ld, const int32_t* __restrict__ labels, int ignore_index, long voxels, int C,
          int count_pos, float* __restrict__ partial) {
  __shared__ int s_lab[kTileV];
  const int t = threadIdx.x;
  const bool dense = ld == C && (((uintptr_t)z) & 15) == 0;   // tile starts are multiples of kTileV * C floats: aligned too
  const float inv_c = 1.f / (float)C;
  BceAcc acc;
  uint32_t nmask = 0, npos = 0, nneg = 0;
  const long ntile = (voxels + kTileV - 1) / kTileV;
  for (long it = blockIdx.x; it < ntile; it += gridDim.x) {
    const long v0 = it * kTileV;
    const int nv = (int)(voxels - v0 < kTileV ? voxels - v0 : kTileV);
    __syncthreads();   // the previous tile's labels have been used
    for (int i = t; i < nv; i += kThreads) {
      const int lab = labels[v0 + i];
      s_lab[i] = lab;
      nmask += lab != ignore_index;
      if (count_pos) {
        if (C == 1) {
          npos += lab == 1;
          nneg += lab == 0;
        } else {
          npos += (unsigned)lab < (unsigned)C;   // neg = C * voxels - pos, formed by the final kernel
        }
      }
    }
    __syncthreads();
    const int nel = nv * C;
    if (dense) {
      const float* zt = z + v0 * C;
      const int nq = nel >> 2;
      for (int q = t; q < nq; q += kThreads) {
        const float4 x4 = reinterpret_cast<const float4*>(zt)[q];
        const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = 4 * q + k, v = elem_voxel(i, inv_c);
          acc.add(xs[k], s_lab[v], i - v * C, C, ignore_index);
        }
      }
      for (int i = 4 * nq + t; i < nel; i += kThreads) {
        const int v = elem_voxel(i, inv_c);
        acc.add(zt[i], s_lab[v], i - v * C, C, ignore_index);
      }
    } else {
      for (int i = t; i < nel; i += kThreads) {
        const int v = elem_voxel(i, inv_c), c = i - v * C;
        acc.add(z[(v0 + v) * ld + c], s_lab[v], c, C, ignore_index);
      }
    }
  }
  // block reduction in a fixed order: shuffle tree per wavefront, then the four wavefronts in order
  __shared__ float sf[kThreads / 64][4];
  __shared__ uint32_t su[kThreads / 64][3];
  const int lane = t & 63, wave = t >> 6;
  float fv[4] = {acc.p, acc.q, acc.yp, acc.yq};
  uint32_t uv[3] = {nmask, npos, nneg};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v = fv[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) sf[wave][k] = v;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    uint32_t v = uv[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) su[wave][k] = v;
  }
  __syncthreads();
  if (t < kNQ) {
    float* rec = partial + (long)blockIdx.x * kNQ;
    if (t < 4) {
      float s = 0.f;
      for (int w = 0; w < kThreads / 64; ++w) s += sf[w][t];
      rec[t] = s;
    } else {
      uint32_t s = 0;
      for (int w = 0; w < kThreads / 64; ++w) s += su[w][t - 4];
      reinterpret_cast<uint32_t*>(rec)[t] = s;
    }
  }
}

// combines the partials in fp64 in a fixed order (the style of loss_final_k): quantity k -> wavefront k, lanes stride
// over the workgroups, fixed-order shuffle tree.  stats = {w_pos, w_neg, pw, scale, sum(l mask), mask, pos, neg}
__global__ void bce_final_k(const float* __restrict__ partial, int nb, long voxels, int C, int weight_mode, int pos_weight_mode,
                            float pos_weight, float* __restrict__ out, double* __restrict__ stats) {
  __shared__ double q[kNQ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (int k = wave; k < kNQ; k += nwaves) {
    double s = 0.0;
#pragma unroll 8
    for (int b = lane; b < nb; b += 64) {
      const float* rec = partial + (long)b * kNQ;
      s += k < 4 ? (double)rec[k] : (double)reinterpret_cast<const uint32_t*>(rec)[k];
    }
    s = msk_wave_sum_d(s);
    if (lane == 0) q[k] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double eps = 1e-10;   // binary_cross_entropy_loss.py:89 self.EPS
  const double nmask = q[4], pos = q[5];
  const double neg = C == 1 ? q[6] : (double)C * (double)voxels - pos;
  const double sum_num = pos + neg + eps;
  double wpos = 1.0, wneg = 1.0, pw = 1.0;
  if (weight_mode == 1) {        // :131-139
    wpos = 2.0 * neg / sum_num;
    wneg = 2.0 * pos / sum_num;
  }
  if (pos_weight_mode == 1) pw = (double)pos_weight;   // :117-119
  else if (pos_weight_mode == 2) pw = 2.0 * neg / sum_num;   // :142-148
  const double sum_l = wneg * (q[0] + pw * q[1]) + (wpos - wneg) * (q[2] + pw * q[3]);
  // :159-160 paddle.mean(loss * mask) / (paddle.mean(mask) + EPS); mask is [N, 1, D, H, W]
  const double scale = 1.0 / ((double)C * (double)voxels) / (nmask / (double)voxels + eps);
  out[0] = (float)(sum_l * scale);
  stats[0] = wpos;
  stats[1] = wneg;
  stats[2] = pw;
  stats[3] = scale;
  stats[4] = sum_l;
  stats[5] = nmask;
  stats[6] = pos;
  stats[7] = neg;
}

// dl/dx = mask w [ (1 - y) sigmoid(x) - pw y sigmoid(-x) ] scale coef  (both sigmoids from e^-|x|: no cancellation)
__device__ __forceinline__ float bce_grad(float x, int lab, int c, int C, int ignore_index, float wpos, float wneg, float pw,
                                          float k) {
  if (lab == ignore_index) return 0.f;
  const float y = bce_target(lab, c, C);
  const float e = expf(-fabsf(x));
  const float big = 1.f / (1.f + e), small = e * big;
  const float sx = x >= 0.f ? big : small, snx = x >= 0.f ? small : big;
  const float w = fmaf(wpos - wneg, y, wneg);
  return w * ((1.f - y) * sx - pw * y * snx) * k;
}

__global__ void __launch_bounds__(kThreads)
bce_bwd_k(const float* __restrict__ z, int ld, const int32_t* __restrict__ labels, int ignore_index,
          const double* __restrict__ stats, float coef, int accumulate, float* __restrict__ dz, int lddz, long voxels, int C) {
  __shared__ int s_lab[kTileV];
  const int t = threadIdx.x;
  const float wpos = (float)stats[0], wneg = (float)stats[1], pw = (float)stats[2];
  const float k = (float)(stats[3] * (double)coef);
  const bool dense = ld == C && lddz == C && ((((uintptr_t)z) | ((uintptr_t)dz)) & 15) == 0;
  const float inv_c = 1.f / (float)C;
  const long ntile = (voxels + kTileV - 1) / kTileV;
  for (long it = blockIdx.x; it < ntile; it += gridDim.x) {
    const long v0 = it * kTileV;
    const int nv = (int)(voxels - v0 < kTileV ? voxels - v0 : kTileV);
    __syncthreads();
    for (int i = t; i < nv; i += kThreads) s_lab[i] = labels[v0 + i];
    __syncthreads();
    const int nel = nv * C;
    if (dense) {
      const float* zt = z + v0 * C;
      float* dt = dz + v0 * C;
      const int nq = nel >> 2;
      for (int q = t; q < nq; q += kThreads) {
        const float4 x4 = reinterpret_cast<const float4*>(zt)[q];
        const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
        float g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = 4 * q + j, v = elem_voxel(i, inv_c);
          g[j] = bce_grad(xs[j], s_lab[v], i - v * C, C, ignore_index, wpos, wneg, pw, k);
        }
        float4 r = make_float4(g[0], g[1], g[2], g[3]);
        if (accumulate) {
          const float4 o = reinterpret_cast<const float4*>(dt)[q];
          r.x += o.x; r.y += o.y; r.z += o.z; r.w += o.w;
        }
        reinterpret_cast<float4*>(dt)[q] = r;
      }
      for (int i = 4 * nq + t; i < nel; i += kThreads) {
        const int v = elem_voxel(i, inv_c);
        const float g = bce_grad(zt[i], s_lab[v], i - v * C, C, ignore_index, wpos, wneg, pw, k);
        dt[i] = accumulate ? dt[i] + g : g;
      }
    } else {
      for (int i = t; i < nel; i += kThreads) {
        const int v = elem_voxel(i, inv_c), c = i - v * C;
        const float g = bce_grad(z[(v0 + v) * ld + c], s_lab[v], c, C, ignore_index, wpos, wneg, pw, k);
        float* dp = dz + (v0 + v) * lddz + c;
        *dp = accumulate ? *dp + g : g;
      }
    }
  }
}

// workgroups of a pass: a fixed function of the shape and the device (bitwise repeatable results), at most 8 per CU
inline int bce_blocks(long voxels, int num_cu) {
  const long tiles = (voxels + kTileV - 1) / kTileV;
  const long cap = 8L * num_cu;
  return (int)(tiles < cap ? tiles : cap);
}

}  // namespace

extern "C" {

int msk_bce_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, int weight_mode, int pos_weight_mode,
                float pos_weight, float* out, double* stats) {
  const int C = logits.c;
  const long voxels = msk_voxels(logits);
  MSK_REQUIRE(ctx, C >= 1 && C <= 64, "num_classes must be in [1,64]");
  MSK_REQUIRE(ctx, logits.ld >= C, "logits.ld must be >= logits.c");
  MSK_REQUIRE(ctx, voxels >= 1 && voxels <= 0x7fffffffL, "voxel count must be in [1, 2^31)");
  MSK_REQUIRE(ctx, weight_mode == 0 || weight_mode == 1, "weight_mode must be 0 (none) or 1 (dynamic)");
  MSK_REQUIRE(ctx, pos_weight_mode >= 0 && pos_weight_mode <= 2, "pos_weight_mode must be 0 (none), 1 (value) or 2 (dynamic)");
  MSK_REQUIRE(ctx, labels != nullptr && out != nullptr && stats != nullptr, "null labels / out / stats");
  const int nb = bce_blocks(voxels, ctx->num_cu);
  float* partial = (float*)msk_workspace(ctx, (size_t)nb * kNQ * sizeof(float));
  if (!partial) return -1;
  const int count_pos = weight_mode == 1 || pos_weight_mode == 2;
  {
    msk_launch_scope ls(ctx, "bce_fwd");
    hipLaunchKernelGGL(bce_fwd_k, dim3(nb), dim3(kThreads), 0, ctx->stream, (const float*)logits.p, logits.ld, labels,
                       ignore_index, voxels, C, count_pos, partial);
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "bce_fwd_final");
    hipLaunchKernelGGL(bce_final_k, dim3(1), dim3(64 * kNQ), 0, ctx->stream, (const float*)partial, nb, voxels, C, weight_mode,
                       pos_weight_mode, pos_weight, out, stats);
    MSK_LAUNCH_CHECK(ctx);
  }
  return 0;
}

int msk_bce_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, const double* stats, float coef,
                int accumulate, msk_tensor dlogits) {
  const int C = logits.c;
  const long voxels = msk_voxels(logits);
  MSK_REQUIRE(ctx, C >= 1 && C <= 64, "num_classes must be in [1,64]");
  MSK_REQUIRE(ctx, logits.ld >= C && dlogits.ld >= C, "ld must be >= c");
  MSK_REQUIRE(ctx, dlogits.c == C && msk_voxels(dlogits) == voxels, "dlogits shape mismatch");
  MSK_REQUIRE(ctx, voxels >= 1 && voxels <= 0x7fffffffL, "voxel count must be in [1, 2^31)");
  MSK_REQUIRE(ctx, labels != nullptr && stats != nullptr, "null labels / stats");
  msk_launch_scope ls(ctx, "bce_bwd");
  hipLaunchKernelGGL(bce_bwd_k, dim3(bce_blocks(voxels, ctx->num_cu)), dim3(kThreads), 0, ctx->stream, (const float*)logits.p,
                     logits.ld, labels, ignore_index, stats, coef, accumulate, (float*)dlogits.p, dlogits.ld, voxels, C);
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
