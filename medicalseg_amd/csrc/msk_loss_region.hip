// Region losses under a mask: soft Dice (nnU-Net's MemoryEfficientSoftDiceLoss / MONAI's DiceLoss options), Tversky, and the
// focal / cross-entropy term, as ONE statistics pass and ONE gradient pass over the logits.  tests/region_reference.py is the
// float64 statement; include/msegk.h gives the formulas and the record layout.
//
//   forward   per (group, class) TP = sum m p t, SP = sum m p^q, ST = sum m t (m = label != ignore_index: the mask multiplies all
//             three, which the V-Net Dice of msk_loss_optim.hip does not do), plus the focal numerator and denominator.  fp32
//             per-thread accumulators, one partial record of 3 C + 2 floats per workgroup, no atomics; region_final_k (one
//             workgroup) merges the records in float64 in a fixed order and evaluates the scores and the two gradient
//             coefficients A, B per (group, class) there, so the backward pass reads finished numbers.
//   backward  recomputes the softmax / sigmoid; dL_r/dp = m (A t + B q p^(q-1)) is linear in A and B, which a workgroup reads once
//             into LDS.
//
// Thread mapping: a thread owns a voxel (its C logits in registers), a workgroup takes tiles of 256 consecutive voxels.  A group
// is the whole batch (batch_dice) or one sample; the tiles of a workgroup never leave its group (grid = groups x workgroups per
// group, a grid-stride loop inside the group), so a partial record belongs to one group and A, B are uniform over a workgroup.
// The logits travel in the three forms of the thread-per-voxel scaffold (tpv_* in msk_device.h, where the rates that fixed each
// form are written down): ST = 2 a flat LDS tile for dense C <= 4, ST = 1 msk_tile_load quads for dense C % 4 == 0, ST = 0 a
// lane's own element loads for channel-slice views (ld > C), unaligned pointers and everything else.
// A masked voxel costs its label only.
#include <cmath>

#include "msk_common.h"

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kTpvThreads, "the tpv_* helpers of msk_device.h assume this workgroup");

struct RegionCfg {
  int ignore_index;
  int sigmoid;   // 0: p = softmax over the classes, 1: p = sigmoid per class
  int squared;   // q == 2
  int focal;     // the focal / CE term is on (softmax only)
  int gmode;     // gamma == 0 (plain CE: no modulating factor at all), 1, 2 (multiplies), 3 = any other value (powf)
  float gamma;
};

struct RegionFin {
  int tversky, do_bg;
  double smooth, alpha, beta;
};

// the class whose target is 1 at a voxel with label y, or one that no class index equals: C == 1 -> t = (y == 1)
__device__ __forceinline__ int region_target_class(int y, int C) { return C == 1 ? (y == 1 ? 0 : -1) : y; }

// zz: logits -> probabilities.  Softmax also returns what the focal term needs: the sum of exponentials, the label's logit less
// the maximum, its probability u, and the sum of the OTHER classes' probabilities (1 - u without a cancellation)
template <int CM>
__device__ __forceinline__ void region_probs(float (&zz)[CM], int C, int y, bool sigmoid, float& se, float& zym, float& u, float& so) {
  float m = -INFINITY;
  se = 0.f; zym = 0.f; u = 0.f; so = 0.f;
  if (sigmoid) {
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) zz[c] = 1.f / (1.f + expf(-zz[c]));
    return;
  }
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) m = fmaxf(m, zz[c]);
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) {
      const float e = expf(zz[c] - m);
      if (c == y) { zym = zz[c] - m; u = e; }
      else so += e;
      se += e;
      zz[c] = e;
    }
  const float inv = 1.f / se;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) zz[c] *= inv;
  so *= inv;
  u *= inv;
}

template <int CM, int ST>
__global__ void __launch_bounds__(kThreads)
region_stats_k(const float* __restrict__ z, int ld, const int32_t* __restrict__ labels, const float* __restrict__ weight,
               RegionCfg cfg, long seg_vox, int wps, int C, float* __restrict__ partial /*[groups * wps][3 C + 2]*/) {
  __shared__ float4 tile[tpv_tile_quads(CM, ST)];
  __shared__ float s_w[CM];
  if (threadIdx.x < CM) s_w[threadIdx.x] = (weight != nullptr && threadIdx.x < C) ? weight[threadIdx.x] : 1.f;
  __syncthreads();
  float aTP[CM], aSP[CM], aST[CM], fnum = 0.f, fden = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c) aTP[c] = aSP[c] = aST[c] = 0.f;
  const int seg = blockIdx.x / wps, first = blockIdx.x - seg * wps;
  const long base = (long)seg * seg_vox;
  const long ntile = (seg_vox + kThreads - 1) / kThreads;
  for (long it = first; it < ntile; it += wps) {
    const long v0 = base + it * kThreads;
    const long left = seg_vox - it * kThreads;
    const int nv = (int)(left < kThreads ? left : kThreads);
    const bool mine = (int)threadIdx.x < nv;
    const long v = v0 + (mine ? threadIdx.x : 0);
    const int y = mine ? labels[v] : cfg.ignore_index;   // asked for ahead of the tile: the two latencies overlap
    tpv_fill<CM, ST>(tile, z + v0 * C, nv, C);
    if (y == cfg.ignore_index) continue;    // m = 0 (or no voxel): adds to nothing (behind the barriers every thread reaches)
    float zz[CM];
    tpv_take<CM, ST>(zz, tile, z + v * ld, C);
    float se, zym, u, so;
    region_probs<CM>(zz, C, y, cfg.sigmoid != 0, se, zym, u, so);
    const int yc = region_target_class(y, C);
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) {
        const float p = zz[c];
        aSP[c] += cfg.squared ? p * p : p;
        if (c == yc) {
          aTP[c] += p;
          aST[c] += 1.f;
        }
      }
    if (cfg.focal && (unsigned)y < (unsigned)C) {
      const float nlogu = logf(se) - zym;   // -log u = -(z_y - max - log sum exp)
      float f = nlogu;
      if (cfg.gmode == 1) f *= so;
      else if (cfg.gmode == 2) f *= so * so;
      else if (cfg.gmode == 3) f *= powf(so, cfg.gamma);
      const float wy = s_w[y];
      fnum = fmaf(wy, f, fnum);
      fden += wy;
    }
  }
  // block reduction: shuffle tree per value, then the four wavefronts' results through LDS (fixed order)
  __shared__ float sh[kThreads / 64][3 * CM + 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto wsum = [](float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  };
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    const float a = wsum(aTP[c]), b = wsum(aSP[c]), t = wsum(aST[c]);
    if (lane == 0) {
      sh[wave][c] = a;
      sh[wave][CM + c] = b;
      sh[wave][2 * CM + c] = t;
    }
  }
  {
    const float a = wsum(fnum), b = wsum(fden);
    if (lane == 0) {
      sh[wave][3 * CM] = a;
      sh[wave][3 * CM + 1] = b;
    }
  }
  __syncthreads();
  const int R = 3 * C + 2;
  for (int i = threadIdx.x; i < R; i += blockDim.x) {
    const int k = i / C, c = i - k * C;
    const int idx = i < 3 * C ? k * CM + c : 3 * CM + (i - 3 * C);   // behind the class sums: the two focal sums
    float v = 0.f;
    for (int w = 0; w < kThreads / 64; ++w) v += sh[w][idx];
    partial[(long)blockIdx.x * R + i] = v;
  }
}

// One workgroup.  Pass 1: the sums, one (quantity, group, class) per wavefront at a time, its 64 lanes stride over the group's
// records in float64 and meet in a fixed-order shuffle tree.  Pass 2: thread c evaluates class c's scores and coefficients
// group by group.  stats = TP[G][C], SP[G][C], ST[G][C], A[G][C], B[G][C], f_num, f_den (doubles)
__global__ void region_final_k(const float* __restrict__ partial, int nseg, int wps, int C, RegionFin fin, float* __restrict__ out,
                               double* __restrict__ stats) {
  __shared__ double s_cls[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int R = 3 * C + 2, GC = nseg * C;
  for (int p = wave; p < 3 * GC + 2; p += nwaves) {
    double s = 0.0;
    int dst;
    if (p < 3 * GC) {
      const int k = p / GC, r = p - k * GC, g = r / C, c = r - g * C;
      const float* rec = partial + (long)g * wps * R + k * C + c;
      for (int b = lane; b < wps; b += 64) s += (double)rec[(long)b * R];
      dst = p;
    } else {
      const int e = p - 3 * GC;
      for (int b = lane; b < nseg * wps; b += 64) s += (double)partial[(long)b * R + 3 * C + e];
      dst = 5 * GC + e;
    }
    s = msk_wave_sum_d(s);
    if (lane == 0) stats[dst] = s;
  }
  __syncthreads();   // (one workgroup: its own global stores are visible behind the barrier)
  const int nscored = (!fin.do_bg && C > 1) ? C - 1 : C;
  const double nk = (double)nseg * (double)nscored;
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    const bool scored = fin.do_bg || C == 1 || c > 0;
    double sum = 0.0;
    for (int g = 0; g < nseg; ++g) {
      const double TP = stats[g * C + c], SP = stats[GC + g * C + c], STt = stats[2 * GC + g * C + c];
      double sc, dTP, dSP;
      if (!fin.tversky) {
        const double num = 2.0 * TP + fin.smooth, raw = SP + STt + fin.smooth;
        const double den = raw > 1e-8 ? raw : 1e-8;
        sc = num / den;
        dTP = 2.0 / den;
        dSP = raw >= 1e-8 ? -num / (den * den) : 0.0;   // the clamp passes no gradient
      } else {
        const double k = 1.0 - fin.alpha - fin.beta;
        const double num = TP + fin.smooth, den = k * TP + fin.alpha * SP + fin.beta * STt + fin.smooth;
        sc = num / den;
        dTP = 1.0 / den - num * k / (den * den);
        dSP = -num * fin.alpha / (den * den);
      }
      stats[3 * GC + g * C + c] = scored ? -dTP / nk : 0.0;
      stats[4 * GC + g * C + c] = scored ? -dSP / nk : 0.0;
      sum += sc;
    }
    out[2 + c] = (float)(sum / (double)nseg);
    s_cls[c] = scored ? sum : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int c = 0; c < C; ++c) tot += s_cls[c];
    const double fn = stats[5 * GC], fd = stats[5 * GC + 1];
    out[0] = (float)(fd != 0.0 ? fn / fd : 0.0);
    out[1] = (float)(1.0 - tot / nk);
  }
}

// registers: see DESIGN.md 7b.  The gradient is formed in place of the probabilities (zz), with dL/dp recomputed in the second
// sweep instead of kept: C registers per voxel, not 3 C.
template <int CM, int ST>
__global__ void __launch_bounds__(kThreads)
region_bwd_k(const float* __restrict__ z, int ld, const int32_t* __restrict__ labels, const float* __restrict__ weight,
             RegionCfg cfg, const double* __restrict__ stats, int nseg, float coef_f, float coef_r, int accumulate,
             float* __restrict__ dz, int lddz, long seg_vox, int wps, int C) {
  __shared__ float4 tile[tpv_tile_quads(CM, ST)];
  __shared__ float s_a[CM], s_b[CM], s_w[CM];
  const int seg = blockIdx.x / wps, first = blockIdx.x - seg * wps;
  const int GC = nseg * C;
  if (threadIdx.x < CM) {
    const int c = threadIdx.x;
    const bool in = c < C;
    // coef_r and q ride in the coefficients: dL_r/dp = a t + b p^(q-1)
    s_a[c] = in ? (float)((double)coef_r * stats[3 * GC + seg * C + c]) : 0.f;
    s_b[c] = in ? (float)((double)coef_r * (cfg.squared ? 2.0 : 1.0) * stats[4 * GC + seg * C + c]) : 0.f;
    s_w[c] = (in && weight != nullptr) ? weight[c] : 1.f;
  }
  const double fden = stats[5 * GC + 1];
  const float kf = (cfg.focal && fden != 0.0) ? (float)((double)coef_f / fden) : 0.f;
  __syncthreads();
  const long base = (long)seg * seg_vox;
  const long ntile = (seg_vox + kThreads - 1) / kThreads;
  for (long it = first; it < ntile; it += wps) {
    const long v0 = base + it * kThreads;
    const long left = seg_vox - it * kThreads;
    const int nv = (int)(left < kThreads ? left : kThreads);
    const bool mine = (int)threadIdx.x < nv;
    const long v = v0 + (mine ? threadIdx.x : 0);
    const int y = mine ? labels[v] : cfg.ignore_index;   // asked for ahead of the tile: the two latencies overlap
    if (ST) {            // tpv_fill's text: the call costs region_bwd_k<12, 0> a register
      __syncthreads();   // the previous tile's store pass is done
      if (ST == 2) tile_load_flat(z + v0 * C, nv * C, reinterpret_cast<float*>(tile));
      else msk_tile_load(z + v0 * C, nv * (C >> 2), C >> 2, tpv_pitch(CM), tile);
      __syncthreads();
    }
    if (!ST && !mine) continue;
    float zz[CM];
    if (y == cfg.ignore_index) {             // m = 0 (or no voxel): the gradient is exactly 0
#pragma unroll
      for (int c = 0; c < CM; ++c) zz[c] = 0.f;
    } else {
      tpv_take<CM, ST>(zz, tile, z + v * ld, C);
      float se, zym, u, so;
      region_probs<CM>(zz, C, y, cfg.sigmoid != 0, se, zym, u, so);
      const int yc = region_target_class(y, C);
      if (cfg.sigmoid) {
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < C) {
            const float p = zz[c];
            const float gp = (c == yc ? s_a[c] : 0.f) + (cfg.squared ? s_b[c] * p : s_b[c]);
            zz[c] = p * (1.f - p) * gp;
          }
      } else {
        // the focal term: w_y (u f'(u)) / den (t - p), u f'(u) = gamma (1-u)^(gamma-1) u log u - (1-u)^gamma
        float kfw = 0.f;
        if (cfg.focal && (unsigned)y < (unsigned)C) {
          float uf = -1.f;                   // gamma == 0
          if (cfg.gmode) {
            const float logu = zym - logf(se);
            const float pg = cfg.gmode == 1 ? 1.f : (cfg.gmode == 2 ? so : powf(so, cfg.gamma - 1.f));
            uf = pg * (cfg.gamma * u * logu - so);
          }
          kfw = kf * s_w[y] * uf;
        }
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < C) {
            const float p = zz[c];
            const float gp = (c == yc ? s_a[c] : 0.f) + (cfg.squared ? s_b[c] * p : s_b[c]);
            dot = fmaf(gp, p, dot);
          }
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < C) {
            const float p = zz[c];
            const float gp = (c == yc ? s_a[c] : 0.f) + (cfg.squared ? s_b[c] * p : s_b[c]);
            zz[c] = fmaf(p, gp - dot, kfw * ((c == yc ? 1.f : 0.f) - p));   // p (g - sum_k p_k g_k) + focal
          }
      }
    }
    if (ST) {
      tpv_put<CM, ST>(zz, tile, dz + v0 * C, C, nv, mine, accumulate != 0);
    } else {
      float* dp = dz + v * lddz;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) dp[c] = accumulate ? dp[c] + zz[c] : zz[c];
    }
  }
}

struct RegionPlan {
  int nseg;       // groups: 1 (batch_dice) or N
  long seg_vox;   // voxels of a group
  int wps;        // workgroups per group
  int st;         // load / store form
};

// per_cu: workgroups per CU in all (3 for the statistics pass: more records only lengthen the one-workgroup merge; 16 for the
// gradient pass).  A fixed function of the shape and the device: results repeat bit for bit.
inline RegionPlan region_plan(const msk_tensor& t, bool dense, int batch_dice, int num_cu, int per_cu) {
  RegionPlan p;
  const long voxels = msk_voxels(t);
  p.nseg = batch_dice ? 1 : t.n;
  p.seg_vox = voxels / p.nseg;
  const long tiles = (p.seg_vox + kThreads - 1) / kThreads;
  long w = (long)num_cu * per_cu / p.nseg;
  if (w > tiles) w = tiles;
  p.wps = (int)(w < 1 ? 1 : w);
  const int C = t.c;
  // a group that starts inside a 16-byte quad cannot take the flat tile's float4 accesses (quad records: C % 4 == 0, never)
  const bool seg_aligned = p.nseg == 1 || (p.seg_vox * C) % 4 == 0;
  p.st = !dense ? 0 : (C <= 4 ? (seg_aligned ? 2 : 0) : ((C % 4 == 0 && C <= 32) ? 1 : 0));
  return p;
}

inline int region_gmode(float gamma) { return gamma == 0.f ? 0 : (gamma == 1.f ? 1 : (gamma == 2.f ? 2 : 3)); }

// the checks both entry points share; 0 = fine
int region_check(msk_ctx* ctx, const msk_tensor& logits, const int32_t* labels, int activation, int squared_pred, int mode,
                 float smooth, float alpha, float beta, int focal_on, float gamma) {
  const int C = logits.c;
  MSK_REQUIRE(ctx, logits.p != nullptr && labels != nullptr, "null logits / labels");
  MSK_REQUIRE(ctx, C >= 1 && C <= 64, "num_classes must be in [1,64]");
  MSK_REQUIRE(ctx, logits.ld >= C, "logits.ld must be >= logits.c");
  MSK_REQUIRE(ctx, logits.n >= 1 && msk_voxels(logits) >= 1 && msk_voxels(logits) <= 0x7fffffffL, "voxel count must be in [1, 2^31)");
  MSK_REQUIRE(ctx, activation == 0 || activation == 1, "activation must be 0 (softmax) or 1 (sigmoid)");
  MSK_REQUIRE(ctx, !(activation == 0 && C == 1), "softmax needs at least 2 classes");
  MSK_REQUIRE(ctx, !(focal_on && activation != 0), "the focal / CE term needs the softmax activation");
  MSK_REQUIRE(ctx, mode == 0 || mode == 1, "mode must be 0 (Dice) or 1 (Tversky)");
  MSK_REQUIRE(ctx, !(mode == 1 && squared_pred), "Tversky does not take squared_pred");
  MSK_REQUIRE(ctx, gamma == 0.f || gamma >= 1.f, "gamma must be 0 or >= 1");
  MSK_REQUIRE(ctx, smooth >= 0.f, "smooth must be >= 0");
  MSK_REQUIRE(ctx, mode == 0 || (alpha >= 0.f && beta >= 0.f), "alpha and beta must be >= 0");
  return 0;
}

}  // namespace

// CM: register arrays sized to the class count in steps of a quad, as the CE + Dice kernels do; 33..64 classes take the
// lane's-own-loads form only (a quad tile of 64 classes would be 68 KiB of LDS)
#define REGION_DISPATCH(LAUNCH)                                        \
  do {                                                                 \
    if (C <= 4) { if (plan.st == 2) LAUNCH(4, 2); else LAUNCH(4, 0); } \
    else if (C <= 32) MSK_TPV_LADDER(C, plan.st == 1, LAUNCH);         \
    else LAUNCH(64, 0);                                                \
  } while (0)

extern "C" {

int msk_region_loss_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, int activation, int squared_pred,
                        int batch_dice, int do_bg, int mode, float smooth, float alpha, float beta, int focal_on, float gamma,
                        const float* weight, float* out, double* stats) {
  if (region_check(ctx, logits, labels, activation, squared_pred, mode, smooth, alpha, beta, focal_on, gamma)) return -1;
  MSK_REQUIRE(ctx, out != nullptr && stats != nullptr, "null out / stats");
  const int C = logits.c;
  const RegionPlan plan = region_plan(logits, msk_quad_dense(logits), batch_dice, ctx->num_cu, 3);
  const int nb = plan.nseg * plan.wps;
  float* partial = (float*)msk_workspace(ctx, (size_t)nb * (3 * C + 2) * sizeof(float));
  if (!partial) return -1;
  const RegionCfg cfg = {ignore_index, activation, squared_pred != 0, focal_on != 0, region_gmode(gamma), gamma};
  {
    msk_launch_scope ls(ctx, "region_fwd_stats");
#define REGION_STATS(CM_, ST_)                                                                                                \
  hipLaunchKernelGGL((region_stats_k<CM_, ST_>), dim3(nb), dim3(kThreads), 0, ctx->stream, (const float*)logits.p, logits.ld, \
                     labels, weight, cfg, plan.seg_vox, plan.wps, C, partial)
    REGION_DISPATCH(REGION_STATS);
#undef REGION_STATS
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    const RegionFin fin = {mode, do_bg != 0, (double)smooth, (double)alpha, (double)beta};
    msk_launch_scope ls(ctx, "region_fwd_final");
    hipLaunchKernelGGL(region_final_k, dim3(1), dim3(1024), 0, ctx->stream, (const float*)partial, plan.nseg, plan.wps, C, fin,
                       out, stats);
    MSK_LAUNCH_CHECK(ctx);
  }
  return 0;
}

int msk_region_loss_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, int activation, int squared_pred,
                        int batch_dice, int do_bg, int mode, float smooth, float alpha, float beta, int focal_on, float gamma,
                        const float* weight, const double* stats, float coef_f, float coef_r, int accumulate, msk_tensor dlogits) {
  if (region_check(ctx, logits, labels, activation, squared_pred, mode, smooth, alpha, beta, focal_on, gamma)) return -1;
  (void)do_bg;   // it is in A and B already
  const int C = logits.c;
  MSK_REQUIRE(ctx, stats != nullptr && dlogits.p != nullptr, "null stats / dlogits");
  MSK_REQUIRE(ctx, msk_same_shape(logits, dlogits) && dlogits.ld >= C, "dlogits shape mismatch");
  const RegionPlan plan = region_plan(logits, msk_quad_dense(logits) && msk_quad_dense(dlogits), batch_dice, ctx->num_cu, 16);
  const int nb = plan.nseg * plan.wps;
  const RegionCfg cfg = {ignore_index, activation, squared_pred != 0, focal_on != 0, region_gmode(gamma), gamma};
  msk_launch_scope ls(ctx, "region_bwd");
#define REGION_BWD(CM_, ST_)                                                                                                \
  hipLaunchKernelGGL((region_bwd_k<CM_, ST_>), dim3(nb), dim3(kThreads), 0, ctx->stream, (const float*)logits.p, logits.ld, \
                     labels, weight, cfg, stats, plan.nseg, coef_f, coef_r, accumulate, (float*)dlogits.p, dlogits.ld,      \
                     plan.seg_vox, plan.wps, C)
  REGION_DISPATCH(REGION_BWD);
#undef REGION_BWD
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
