// Region-based training (nnU-Net's DC_and_BCE_loss over label regions): sigmoid Dice + binary cross entropy against MULTI-HOT
// targets, as ONE statistics pass and ONE gradient pass over the logits, and the label map rebuilt from the thresholded channels
// (regions_class_order).  tests/mlabel_reference.py is the float64 statement; include/msegk.h gives the formulas and the record
// layout.
//
// The label stays one int32 per voxel.  table[v] (uint32, v < table_len <= 256) holds the bit mask of the regions label value v
// belongs to: t_r = bit r of table[y], 0 for a label outside the table.  A workgroup copies the table into LDS once (1 KiB).
//
//   forward   per (group, region) TP = sum m p t, SP = sum m p^q, ST = sum m t (m = label != ignore_index), plus the BCE sum
//             sum m sum_r (max(z, 0) - z t + log(1 + exp(-|z|))) and the number of valid voxels.  The sigmoid and the BCE term share
//             one expf(-|z|): p = 1 / (1 + e) or e / (1 + e) by the sign of z, so neither overflows and 1 - p comes without a
//             cancellation; a voxel's R logarithms are one logf of the product of its 1 + e.  fp32 per-thread accumulators, one
//             partial record of 3 R + 2 floats per workgroup, no atomics; mlabel_final_k (one workgroup) merges the records in
//             float64 in a fixed order and evaluates the scores and the gradient coefficients A, B per (group, region).
//   backward  recomputes the sigmoid; dL/dz = kb m (p - t) + m (A t + B q p^(q-1)) p (1 - p), kb = coef_bce / (R sum m).
//
// Thread mapping: that of msk_loss_region.hip.  A thread owns a voxel (its R logits in registers), a workgroup takes tiles of 256
// consecutive voxels inside one group (the batch with batch_dice, else a sample), grid = groups x workgroups per group.  The logits
// travel in the three forms of the thread-per-voxel scaffold (tpv_* in msk_device.h): ST = 2 a flat LDS tile for dense R <= 4,
// ST = 1 quad tiles for dense R % 4 == 0, ST = 0 a lane's own loads for channel-slice views, unaligned pointers and unaligned
// group starts.  R <= 32: there is no 64-wide form.  The label is asked for ahead of the tile barrier; a masked voxel costs its
// label only.
#include <cmath>

#include "msk_common.h"

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kTpvThreads, "the tpv_* helpers of msk_device.h assume this workgroup");
constexpr int kTableMax = 256;
constexpr int kRegionsMax = 32;

struct MlabelCfg {
  int ignore_index;
  int squared;     // q == 2
  int table_len;
};

// e = expf(-|z|) is shared: p = sigmoid(z), omp = 1 - p, ope = 1 + e (the BCE term's log(1 + exp(-|z|)) = log(ope))
__device__ __forceinline__ void mlabel_sigmoid(float z, float& p, float& omp, float& ope) {
  const float e = expf(-fabsf(z));
  ope = 1.f + e;
  // v_rcp_f32 (1 ulp) of a value in [1, 2]: the IEEE division's range fix-up buys nothing here, and its sequence was the larger
  // half of this function (the forward pass missed its mark with it: DESIGN.md 7)
  const float inv = __builtin_amdgcn_rcpf(ope);
  const float ei = e * inv;
  p = z >= 0.f ? inv : ei;
  omp = z >= 0.f ? ei : inv;
}

// the table into LDS, one entry per thread, entries past table_len zero: a label in [table_len, 256) reads an all-zero row like
// one outside [0, 256).  The load is asked for at the top of the kernel; the store into LDS waits behind the first tile's label
// load in mlabel_stats_k (ahead of a barrier every thread reaches), so the two latencies overlap.
static_assert(kTableMax == kThreads, "one table entry per thread");
__device__ __forceinline__ uint32_t mlabel_table_get(const uint32_t* __restrict__ table, int table_len) {
  return (int)threadIdx.x < table_len ? table[threadIdx.x] : 0u;
}
__device__ __forceinline__ uint32_t mlabel_bits(const uint32_t* __restrict__ s_tab, int y) {
  return (unsigned)y < (unsigned)kTableMax ? s_tab[y] : 0u;
}

template <int CM, int ST>
__global__ void __launch_bounds__(kThreads)
mlabel_stats_k(const float* __restrict__ z, int ld, const int32_t* __restrict__ labels, const uint32_t* __restrict__ table,
               MlabelCfg cfg, long seg_vox, int wps, int C, float* __restrict__ partial /*[groups * wps][3 C + 2]*/) {
  __shared__ float4 tile[tpv_tile_quads(CM, ST)];
  __shared__ uint32_t s_tab[kTableMax];
  const uint32_t tv = mlabel_table_get(table, cfg.table_len);
  float aTP[CM], aSP[CM], aST[CM], bsum = 0.f, cnt = 0.f;
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
    if (it == first) {                      // uniform over the workgroup; the tile forms' own barriers publish the table
      s_tab[threadIdx.x] = tv;
      if (!ST) __syncthreads();
    }
    tpv_fill<CM, ST>(tile, z + v0 * C, nv, C);
    if (y == cfg.ignore_index) continue;    // m = 0 (or no voxel): adds to nothing (behind the barriers every thread reaches)
    float zz[CM];
    tpv_take<CM, ST>(zz, tile, z + v * ld, C);
    const uint32_t tb = mlabel_bits(s_tab, y);
    // sum_r log(1 + e_r) = log(prod_r (1 + e_r)): every factor lies in [1, 2], so 32 of them stay below 2^32 and a voxel
    // costs ONE logf, not R
    float bs = 0.f, prod = 1.f;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) {
        const float zc = zz[c];
        float p, omp, ope;
        mlabel_sigmoid(zc, p, omp, ope);
        const bool t = (tb >> c) & 1u;
        aSP[c] += cfg.squared ? p * p : p;
        if (t) {
          aTP[c] += p;
          aST[c] += 1.f;
        }
        bs += fmaxf(t ? -zc : zc, 0.f);         // max(z, 0) - z t for t in {0, 1}
        prod *= ope;
      }
    bsum += bs + logf(prod);
    cnt += 1.f;
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
    const float a = wsum(bsum), b = wsum(cnt);
    if (lane == 0) {
      sh[wave][3 * CM] = a;
      sh[wave][3 * CM + 1] = b;
    }
  }
  __syncthreads();
  const int R = 3 * C + 2;
  for (int i = threadIdx.x; i < R; i += blockDim.x) {
    const int k = i / C, c = i - k * C;
    const int idx = i < 3 * C ? k * CM + c : 3 * CM + (i - 3 * C);   // behind the region sums: the BCE sum and the valid count
    float v = 0.f;
    for (int w = 0; w < kThreads / 64; ++w) v += sh[w][idx];
    partial[(long)blockIdx.x * R + i] = v;
  }
}

// One workgroup.  Pass 1: the sums, one (quantity, group, region) per wavefront at a time, its 64 lanes stride over the group's
// records in float64 and meet in a fixed-order shuffle tree.  Pass 2: thread c evaluates region c's scores and coefficients group
// by group.  stats = TP[G][C], SP[G][C], ST[G][C], A[G][C], B[G][C], bce_sum, valid (doubles)
__global__ void mlabel_final_k(const float* __restrict__ partial, int nseg, int wps, int C, double smooth, float* __restrict__ out,
                               double* __restrict__ stats) {
  __shared__ double s_cls[kRegionsMax];
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
  const double nk = (double)nseg * (double)C;
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    double sum = 0.0;
    for (int g = 0; g < nseg; ++g) {
      const double TP = stats[g * C + c], SP = stats[GC + g * C + c], STt = stats[2 * GC + g * C + c];
      const double num = 2.0 * TP + smooth, raw = SP + STt + smooth;
      const double den = raw > 1e-8 ? raw : 1e-8;
      stats[3 * GC + g * C + c] = -2.0 / (nk * den);
      stats[4 * GC + g * C + c] = raw > 1e-8 ? num / (nk * den * den) : 0.0;   // the clamp passes no gradient
      sum += num / den;
    }
    out[2 + c] = (float)(sum / (double)nseg);
    s_cls[c] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int c = 0; c < C; ++c) tot += s_cls[c];
    const double bs = stats[5 * GC], valid = stats[5 * GC + 1];
    out[0] = (float)(valid != 0.0 ? bs / ((double)C * valid) : 0.0);
    out[1] = (float)(1.0 - tot / nk);
  }
}

template <int CM, int ST>
__global__ void __launch_bounds__(kThreads)
mlabel_bwd_k(const float* __restrict__ z, int ld, const int32_t* __restrict__ labels, const uint32_t* __restrict__ table,
             MlabelCfg cfg, const double* __restrict__ stats, int nseg, float coef_bce, float coef_dice, int accumulate,
             float* __restrict__ dz, int lddz, long seg_vox, int wps, int C) {
  __shared__ float4 tile[tpv_tile_quads(CM, ST)];
  __shared__ uint32_t s_tab[kTableMax];
  __shared__ float s_a[CM], s_b[CM];
  const int seg = blockIdx.x / wps, first = blockIdx.x - seg * wps;
  const int GC = nseg * C;
  s_tab[threadIdx.x] = mlabel_table_get(table, cfg.table_len);
  if (threadIdx.x < CM) {
    const int c = threadIdx.x;
    const bool in = c < C;
    // coef_dice and q ride in the coefficients: dL_dice/dp = a t + b p^(q-1)
    s_a[c] = in ? (float)((double)coef_dice * stats[3 * GC + seg * C + c]) : 0.f;
    s_b[c] = in ? (float)((double)coef_dice * (cfg.squared ? 2.0 : 1.0) * stats[4 * GC + seg * C + c]) : 0.f;
  }
  const double valid = stats[5 * GC + 1];
  const float kb = valid != 0.0 ? (float)((double)coef_bce / ((double)C * valid)) : 0.f;
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
    tpv_fill<CM, ST>(tile, z + v0 * C, nv, C);
    if (!ST && !mine) continue;
    float zz[CM];
    if (y == cfg.ignore_index) {             // m = 0 (or no voxel): the gradient is exactly 0
#pragma unroll
      for (int c = 0; c < CM; ++c) zz[c] = 0.f;
    } else {
      tpv_take<CM, ST>(zz, tile, z + v * ld, C);
      const uint32_t tb = mlabel_bits(s_tab, y);
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) {
          float p, omp, ope;
          mlabel_sigmoid(zz[c], p, omp, ope);
          const bool t = (tb >> c) & 1u;
          const float gp = (t ? s_a[c] : 0.f) + (cfg.squared ? s_b[c] * p : s_b[c]);
          zz[c] = kb * (t ? -omp : p) + (p * omp) * gp;   // p - 1 = -(1 - p): no cancellation under a target of 1
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

struct MlabelPlan {
  int nseg;       // groups: 1 (batch_dice) or N
  long seg_vox;   // voxels of a group
  int wps;        // workgroups per group
  int st;         // load / store form
};

// per_cu: workgroups per CU in all (3 for the statistics pass: more records only lengthen the one-workgroup merge; 16 for the
// gradient pass), the rule of region_plan.  A fixed function of the shape and the device: results repeat bit for bit.
inline MlabelPlan mlabel_plan(const msk_tensor& t, bool dense, int batch_dice, int num_cu, int per_cu) {
  MlabelPlan p;
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
  p.st = !dense ? 0 : (C <= 4 ? (seg_aligned ? 2 : 0) : (C % 4 == 0 ? 1 : 0));
  return p;
}

// bytes from a tensor's first element to behind its last
inline size_t mlabel_span(const msk_tensor& t) { return ((size_t)(msk_voxels(t) - 1) * (size_t)t.ld + (size_t)t.c) * sizeof(float); }

// the checks both loss entry points share; 0 = fine
int mlabel_check(msk_ctx* ctx, const msk_tensor& logits, const int32_t* labels, const uint32_t* table, int table_len, float smooth) {
  MSK_REQUIRE(ctx, logits.p != nullptr && labels != nullptr && table != nullptr, "null logits / labels / table");
  MSK_REQUIRE(ctx, (((uintptr_t)logits.p) & 3) == 0 && (((uintptr_t)labels) & 3) == 0 && (((uintptr_t)table) & 3) == 0,
              "logits, labels and table must be 4-byte aligned");
  MSK_REQUIRE(ctx, logits.c >= 1 && logits.c <= kRegionsMax, "the number of regions (logits.c) must be in [1,32]");
  MSK_REQUIRE(ctx, table_len >= 1 && table_len <= kTableMax, "table_len must be in [1,256]");
  MSK_REQUIRE(ctx, logits.ld >= logits.c, "logits.ld must be >= logits.c");
  MSK_REQUIRE(ctx, logits.n >= 1 && logits.d >= 1 && logits.h >= 1 && logits.w >= 1 && msk_voxels(logits) < 0x80000000L,
              "voxel count must be in [1, 2^31)");
  MSK_REQUIRE(ctx, smooth >= 0.f, "smooth must be >= 0");
  return 0;
}

struct RegionOrder {
  int32_t v[kRegionsMax];
};

// out = 0, then for r = 0 .. R-1 in order: out = order[r] where z_r > 0 (the last region that fires wins; a NaN does not fire)
__global__ void regions_to_label_k(const float* __restrict__ x, int ld, long voxels, int R, RegionOrder order, int32_t* __restrict__ out) {
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < voxels; v += (long)gridDim.x * blockDim.x) {
    const float* p = x + v * ld;
    int32_t o = 0;
    // four regions per step, their loads issued together (written one by one the compiler waits for every logit before it asks
    // for the next); a step past R - 1 reads logit R - 1 again and takes no part
    for (int r = 0; r < R; r += 4) {
      float q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = p[r + k < R ? r + k : R - 1];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int32_t cls = order.v[r + k < R ? r + k : R - 1];   // a uniform index: a scalar load
        o = (r + k < R && q[k] > 0.f) ? cls : o;
      }
    }
    out[v] = o;
  }
}

}  // namespace

// CM: register arrays sized to the region count in steps of a quad, as the region kernels do
#define MLABEL_DISPATCH(LAUNCH)                                        \
  do {                                                                 \
    if (C <= 4) { if (plan.st == 2) LAUNCH(4, 2); else LAUNCH(4, 0); } \
    else MSK_TPV_LADDER(C, plan.st == 1, LAUNCH);                      \
  } while (0)

extern "C" {

int msk_mlabel_loss_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, const uint32_t* table,
                        int table_len, int squared_pred, int batch_dice, float smooth, float* out, double* stats) {
  if (mlabel_check(ctx, logits, labels, table, table_len, smooth)) return -1;
  MSK_REQUIRE(ctx, out != nullptr && stats != nullptr, "null out / stats");
  MSK_REQUIRE(ctx, (((uintptr_t)out) & 3) == 0 && (((uintptr_t)stats) & 7) == 0, "out must be 4-byte, stats 8-byte aligned");
  const int C = logits.c;
  const MlabelPlan plan = mlabel_plan(logits, msk_quad_dense(logits), batch_dice, ctx->num_cu, 3);
  const int nb = plan.nseg * plan.wps;
  float* partial = (float*)msk_workspace(ctx, (size_t)nb * (3 * C + 2) * sizeof(float));
  if (!partial) return -1;
  const MlabelCfg cfg = {ignore_index, squared_pred != 0, table_len};
  {
    msk_launch_scope ls(ctx, "mlabel_fwd_stats");
#define MLABEL_STATS(CM_, ST_)                                                                                                \
  hipLaunchKernelGGL((mlabel_stats_k<CM_, ST_>), dim3(nb), dim3(kThreads), 0, ctx->stream, (const float*)logits.p, logits.ld, \
                     labels, table, cfg, plan.seg_vox, plan.wps, C, partial)
    MLABEL_DISPATCH(MLABEL_STATS);
#undef MLABEL_STATS
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "mlabel_fwd_final");
    hipLaunchKernelGGL(mlabel_final_k, dim3(1), dim3(1024), 0, ctx->stream, (const float*)partial, plan.nseg, plan.wps, C,
                       (double)smooth, out, stats);
    MSK_LAUNCH_CHECK(ctx);
  }
  return 0;
}

int msk_mlabel_loss_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, const uint32_t* table,
                        int table_len, int squared_pred, int batch_dice, float smooth, const double* stats, float coef_bce,
                        float coef_dice, int accumulate, msk_tensor dlogits) {
  if (mlabel_check(ctx, logits, labels, table, table_len, smooth)) return -1;
  const int C = logits.c;
  MSK_REQUIRE(ctx, stats != nullptr && dlogits.p != nullptr, "null stats / dlogits");
  MSK_REQUIRE(ctx, (((uintptr_t)stats) & 7) == 0 && (((uintptr_t)dlogits.p) & 3) == 0, "stats must be 8-byte, dlogits 4-byte aligned");
  MSK_REQUIRE(ctx, msk_same_shape(logits, dlogits) && dlogits.ld >= C, "dlogits shape mismatch");
  MSK_REQUIRE(ctx, msk_bytes_disjoint(logits.p, mlabel_span(logits), dlogits.p, mlabel_span(dlogits)), "dlogits overlaps the logits");
  const MlabelPlan plan = mlabel_plan(logits, msk_quad_dense(logits) && msk_quad_dense(dlogits), batch_dice, ctx->num_cu, 16);
  const int nb = plan.nseg * plan.wps;
  const MlabelCfg cfg = {ignore_index, squared_pred != 0, table_len};
  msk_launch_scope ls(ctx, "mlabel_bwd");
#define MLABEL_BWD(CM_, ST_)                                                                                                \
  hipLaunchKernelGGL((mlabel_bwd_k<CM_, ST_>), dim3(nb), dim3(kThreads), 0, ctx->stream, (const float*)logits.p, logits.ld, \
                     labels, table, cfg, stats, plan.nseg, coef_bce, coef_dice, accumulate, (float*)dlogits.p, dlogits.ld,  \
                     plan.seg_vox, plan.wps, C)
  MLABEL_DISPATCH(MLABEL_BWD);
#undef MLABEL_BWD
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

int msk_regions_to_label(msk_ctx* ctx, msk_tensor logits, const int32_t* class_order, int32_t* out) {
  MSK_REQUIRE(ctx, logits.p != nullptr && class_order != nullptr && out != nullptr, "null logits / class_order / out");
  MSK_REQUIRE(ctx, (((uintptr_t)logits.p) & 3) == 0 && (((uintptr_t)out) & 3) == 0, "logits and out must be 4-byte aligned");
  MSK_REQUIRE(ctx, logits.c >= 1 && logits.c <= kRegionsMax, "the number of regions (logits.c) must be in [1,32]");
  MSK_REQUIRE(ctx, logits.ld >= logits.c, "logits.ld must be >= logits.c");
  MSK_REQUIRE(ctx, logits.n >= 1 && logits.d >= 1 && logits.h >= 1 && logits.w >= 1 && msk_voxels(logits) < 0x80000000L,
              "voxel count must be in [1, 2^31)");
  const long voxels = msk_voxels(logits);
  RegionOrder order;
  for (int r = 0; r < kRegionsMax; ++r) order.v[r] = r < logits.c ? class_order[r] : 0;   // by value in the kernel arguments
  int cap = 4;
  msk_get_ew_option("ew_cap", &cap);   // the grid of msk_argmax_c
  msk_launch_scope ls(ctx, "regions_to_label");
  hipLaunchKernelGGL(regions_to_label_k, dim3(msk_ew_blocks(voxels, ctx->num_cu, cap)), dim3(kThreads), 0, ctx->stream,
                     (const float*)logits.p, logits.ld, voxels, logits.c, order, out);
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
