// Boundary loss (Kervadec et al., MIDL 2019; the BDLoss / DC_and_BD_loss of the nnU-Net loss collections): the softmax
// probability times the signed distance map of the ground truth, averaged -- with the map BUILT ON THE DEVICE from the label patch
// by the exact distance transform of msk_edt.hip.  tests/boundary_reference.py is the statement; include/msegk.h gives the
// formulas and the record layout.
//
//   map       msk_label_sdf: per (volume, class of the set) two exact transforms into the two float64 fields of the workspace --
//             features {== c}: d_out^2, the squared distance to the class; features {!= c}: d_in^2, the squared distance to its
//             complement, from the complemented x pass of msk_edt.hip (no mask volume is written) -- and ONE compose pass
//             (sdf_compose_k): phi = sqrt(d_out^2) outside the class, 1 - sqrt(d_in^2) inside (float64, correctly rounded square
//             root; a voxel with d_in = 1 gets +0.0), 0 where the squared distance is +inf (class absent / class fills the volume),
//             rounded once to float32.  Reads 4 + 8 + 8 bytes and writes 4 bytes per voxel.  Seven launches per (volume, class)
//             on the context stream, the fields reused from one to the next.  phi is class-planar: plane (n |S| + j) holds the
//             j-th set bit of class_mask.
//   forward   boundary_stats_k: a thread owns a voxel (the thread-per-voxel scaffold of msk_device.h, the three record forms of
//             msk_loss_region.hip), t_c = p_c phi_c for the classes of the set at the valid voxels.  A lane reads its label and its
//             |S| phi values (coalesced per plane: consecutive lanes, consecutive floats) AHEAD of the tile barrier.  fp32
//             per-thread sums, one record {sum t_c [C], sum |t|, n_valid (an integer's bits)} per workgroup, no atomics;
//             boundary_final_k (one workgroup) merges the records in float64 in a fixed order: two calls give the same bits.
//   backward  boundary_bwd_k recomputes the softmax: dz_k (+)= coef p_k ([k in S] phi_k - sum_c t_c) / (n_valid |S|); n_valid is
//             read from the forward's record behind the first tile's label and phi loads.  Invalid voxels: exact zeros, or
//             nothing at all when the pass adds.
// The workgroups of a launch never leave their sample (grid = samples x workgroups per sample), so the phi planes of a workgroup
// are those of one sample.
#include <cmath>

#include "msk_common.h"

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kTpvThreads, "the tpv_* helpers of msk_device.h assume this workgroup");
constexpr int kMaxExtent = MSK_EDT_MAX_EXTENT;

inline size_t sdf_round256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t sdf_ws_bytes(long V) { return 2 * sdf_round256((size_t)V * sizeof(double)); }

// grid-stride over the voxels of one volume
__global__ void __launch_bounds__(kThreads)
sdf_compose_k(const int32_t* __restrict__ lab, const double* __restrict__ d2_out, const double* __restrict__ d2_in, int cls, long V,
              float* __restrict__ phi) {
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < V; i += (long)gridDim.x * kThreads) {
    const bool inside = lab[i] == cls;
    const double q = inside ? d2_in[i] : d2_out[i];
    double r = 0.0;
    if (q < inf) {
      const double s = sqrt(q);   // correctly rounded, as msk_fg_stats' std field is held to numpy's bits
      r = inside ? 1.0 - s : s;
    }
    phi[i] = (float)r;
  }
}

// zz: logits -> softmax probabilities (the arithmetic of region_probs)
template <int CM>
__device__ __forceinline__ void boundary_probs(float (&zz)[CM], int C) {
  float m = -INFINITY, se = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) m = fmaxf(m, zz[c]);
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) {
      zz[c] = expf(zz[c] - m);
      se += zz[c];
    }
  const float inv = 1.f / se;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) zz[c] *= inv;
}

// this voxel's phi of every class of the set (0 elsewhere): pv = its float in the first plane of its sample, planes V apart
template <int CM>
__device__ __forceinline__ void boundary_phi(float (&ph)[CM], const float* __restrict__ pv, long V, uint64_t mask, bool mine) {
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    ph[c] = 0.f;
    if ((mask >> c) & 1) {   // uniform
      if (mine) ph[c] = *pv;
      pv += V;
    }
  }
}

template <int CM, int ST>
__global__ void __launch_bounds__(kThreads)
boundary_stats_k(const float* __restrict__ z, int ld, const int32_t* __restrict__ labels, const float* __restrict__ phi,
                 int ignore_index, uint64_t mask, int nset, long V, int wps, int C, float* __restrict__ partial /*[nb][C + 2]*/) {
  __shared__ float4 tile[tpv_tile_quads(CM, ST)];
  float acc[CM], aabs = 0.f;
  uint32_t nvalid = 0;
#pragma unroll
  for (int c = 0; c < CM; ++c) acc[c] = 0.f;
  const int seg = blockIdx.x / wps, first = blockIdx.x - seg * wps;
  const long base = (long)seg * V;
  const float* phis = phi + (long)seg * nset * V;
  const long ntile = (V + kThreads - 1) / kThreads;
  for (long it = first; it < ntile; it += wps) {
    const long r0 = it * kThreads;
    const long left = V - r0;
    const int nv = (int)(left < kThreads ? left : kThreads);
    const bool mine = (int)threadIdx.x < nv;
    const long r = r0 + (mine ? threadIdx.x : 0);
    const long v = base + r;
    // asked for ahead of the tile: the latencies overlap
    const int y = mine ? labels[v] : ignore_index;
    float ph[CM];
    boundary_phi<CM>(ph, phis + r, V, mask, mine);
    tpv_fill<CM, ST>(tile, z + (base + r0) * C, nv, C);
    if (!mine || y == ignore_index || (unsigned)y >= (unsigned)C) continue;   // behind the barriers every thread reaches
    float zz[CM];
    tpv_take<CM, ST>(zz, tile, z + v * ld, C);
    boundary_probs<CM>(zz, C);
    ++nvalid;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if ((mask >> c) & 1) {
        const float t = zz[c] * ph[c];
        acc[c] += t;
        aabs += fabsf(t);
      }
  }
  // block reduction: shuffle tree per value, then the four wavefronts' results through LDS (fixed order)
  __shared__ float sh[kThreads / 64][CM + 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto wsum = [](float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  };
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    const float a = wsum(acc[c]);
    if (lane == 0) sh[wave][c] = a;
  }
  {
    const float a = wsum(aabs);
    const uint32_t n = msk_wave_sum_u32(nvalid);
    if (lane == 0) {
      sh[wave][CM] = a;
      sh[wave][CM + 1] = __uint_as_float(n);
    }
  }
  __syncthreads();
  const int R = C + 2;
  for (int i = threadIdx.x; i < R; i += blockDim.x) {
    const int idx = i < C ? i : CM + (i - C);
    float out;
    if (i == C + 1) {
      uint32_t n = 0;
      for (int w = 0; w < kThreads / 64; ++w) n += __float_as_uint(sh[w][idx]);
      out = __uint_as_float(n);
    } else {
      float s = 0.f;
      for (int w = 0; w < kThreads / 64; ++w) s += sh[w][idx];
      out = s;
    }
    partial[(long)blockIdx.x * R + i] = out;
  }
}

// One workgroup.  Pass 1: one quantity per wavefront at a time, its 64 lanes stride over the nb records in float64 (n_valid:
// integers, exact) and meet in a fixed-order shuffle tree.  Pass 2: the record and out.
// stats = {n_valid, sum t, sum |t|, sum t_c [C]};  out = {L, A, L_c [C]}
__global__ void boundary_final_k(const float* __restrict__ partial, int nb, int C, int nset, float* __restrict__ out,
                                 double* __restrict__ stats) {
  __shared__ double s_q[64 + 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int R = C + 2;
  for (int q = wave; q < R; q += nwaves) {
    double s = 0.0;
    if (q == C + 1) {
      for (int b = lane; b < nb; b += 64) s += (double)__float_as_uint(partial[(long)b * R + q]);
    } else {
      for (int b = lane; b < nb; b += 64) s += (double)partial[(long)b * R + q];
    }
    s = msk_wave_sum_d(s);
    if (lane == 0) s_q[q] = s;
  }
  __syncthreads();
  const double nvalid = s_q[C + 1];
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    stats[3 + c] = s_q[c];
    out[2 + c] = nvalid > 0.0 ? (float)(s_q[c] / nvalid) : 0.f;
  }
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int c = 0; c < C; ++c) tot += s_q[c];
    const double den = nvalid * (double)nset;
    stats[0] = nvalid;
    stats[1] = tot;
    stats[2] = s_q[C];
    out[0] = nvalid > 0.0 ? (float)(tot / den) : 0.f;
    out[1] = nvalid > 0.0 ? (float)(s_q[C] / den) : 0.f;
  }
}

// registers: see DESIGN.md 7c.  The gradient is formed in place of the probabilities (zz).
template <int CM, int ST>
__global__ void __launch_bounds__(kThreads)
boundary_bwd_k(const float* __restrict__ z, int ld, const int32_t* __restrict__ labels, const float* __restrict__ phi, int ignore_index,
               uint64_t mask, int nset, const double* __restrict__ stats, float coef, int accumulate, float* __restrict__ dz, int lddz,
               long V, int wps, int C) {
  __shared__ float4 tile[tpv_tile_quads(CM, ST)];
  const int seg = blockIdx.x / wps, first = blockIdx.x - seg * wps;
  const long base = (long)seg * V;
  const float* phis = phi + (long)seg * nset * V;
  const long ntile = (V + kThreads - 1) / kThreads;
  float scale = 0.f;
  bool have_scale = false;
  for (long it = first; it < ntile; it += wps) {
    const long r0 = it * kThreads;
    const long left = V - r0;
    const int nv = (int)(left < kThreads ? left : kThreads);
    const bool mine = (int)threadIdx.x < nv;
    const long r = r0 + (mine ? threadIdx.x : 0);
    const long v = base + r;
    // asked for ahead of the tile (and, in the first round, ahead of the forward's record): the latencies overlap
    const int y = mine ? labels[v] : ignore_index;
    float ph[CM];
    boundary_phi<CM>(ph, phis + r, V, mask, mine);
    if (!have_scale) {
      const double nvalid = stats[0];
      scale = nvalid > 0.0 ? (float)((double)coef / (nvalid * (double)nset)) : 0.f;
      have_scale = true;
    }
    tpv_fill<CM, ST>(tile, z + (base + r0) * C, nv, C);
    if (!ST && !mine) continue;
    const bool valid = mine && y != ignore_index && (unsigned)y < (unsigned)C;
    float zz[CM];
    if (!valid) {                              // the gradient is exactly 0
#pragma unroll
      for (int c = 0; c < CM; ++c) zz[c] = 0.f;
    } else {
      tpv_take<CM, ST>(zz, tile, z + v * ld, C);
      boundary_probs<CM>(zz, C);
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if ((mask >> c) & 1) dot = fmaf(zz[c], ph[c], dot);
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) zz[c] = scale * (zz[c] * (ph[c] - dot));
    }
    if (ST) {
      tpv_put<CM, ST>(zz, tile, dz + (base + r0) * C, C, nv, mine, accumulate != 0);
    } else if (!(accumulate && !valid)) {      // an invalid voxel of an adding pass is left as it is
      float* dp = dz + v * lddz;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) dp[c] = accumulate ? dp[c] + zz[c] : zz[c];
    }
  }
}

struct BoundaryPlan {
  long V;     // voxels of a sample
  int wps;    // workgroups per sample
  int st;     // load / store form
  int nset;   // |S|
};

// per_cu: workgroups per CU in all (3 for the statistics pass: more records only lengthen the one-workgroup merge; 16 for the
// gradient pass).  A fixed function of the shape and the device: results repeat bit for bit.
inline BoundaryPlan boundary_plan(const msk_tensor& t, bool dense, uint64_t mask, int num_cu, int per_cu) {
  BoundaryPlan p;
  p.V = (long)t.d * t.h * t.w;
  const long tiles = (p.V + kThreads - 1) / kThreads;
  long w = (long)num_cu * per_cu / t.n;
  if (w > tiles) w = tiles;
  p.wps = (int)(w < 1 ? 1 : w);
  const int C = t.c;
  // a sample that starts inside a 16-byte quad cannot take the flat tile's float4 accesses (quad records: C % 4 == 0, never)
  const bool seg_aligned = t.n == 1 || (p.V * C) % 4 == 0;
  p.st = !dense ? 0 : (C <= 4 ? (seg_aligned ? 2 : 0) : ((C % 4 == 0 && C <= 32) ? 1 : 0));
  p.nset = __builtin_popcountll(mask);
  return p;
}

// N V < 2^31, by division (the product of four extents need not fit 64 bits' worth of care: V <= 2^33 does)
inline bool boundary_count_ok(int n, int d, int h, int w) {
  if (n < 1 || d < 1 || h < 1 || w < 1 || d > kMaxExtent || h > kMaxExtent || w > kMaxExtent) return false;
  const long V = (long)d * h * w;
  return (long)n <= 0x7fffffffL / V;
}

inline size_t tensor_bytes(const msk_tensor& t) { return ((size_t)(msk_voxels(t) - 1) * t.ld + t.c) * sizeof(float); }

// the checks both loss entry points share; 0 = fine
int boundary_check(msk_ctx* ctx, const msk_tensor& logits, const int32_t* labels, uint64_t mask, const float* phi) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, logits.p != nullptr && labels != nullptr && phi != nullptr, "null logits / labels / phi");
  const int C = logits.c;
  MSK_REQUIRE(ctx, C >= 2 && C <= 64, "num_classes must be in [2,64]");
  MSK_REQUIRE(ctx, logits.ld >= C, "logits.ld must be >= logits.c");
  MSK_REQUIRE(ctx, mask != 0 && (C == 64 || (mask >> C) == 0), "class_mask must name at least one class and none >= num_classes");
  MSK_REQUIRE(ctx, boundary_count_ok(logits.n, logits.d, logits.h, logits.w),
              "every extent must be in [1, 2048] (MSK_EDT_MAX_EXTENT) and the voxel count below 2^31");
  MSK_REQUIRE(ctx, ((((uintptr_t)logits.p) | ((uintptr_t)labels)) & 3) == 0, "logits / labels must be 4-byte aligned");
  MSK_REQUIRE(ctx, (((uintptr_t)phi) & 15) == 0, "phi must be 16-byte aligned");
  return 0;
}

}  // namespace

// CM: register arrays sized to the class count in steps of a quad, as the region kernels do; 33..64 classes take the lane's-own
// form only (no LDS tile)
#define BOUNDARY_DISPATCH(LAUNCH)                                      \
  do {                                                                 \
    if (C <= 4) { if (plan.st == 2) LAUNCH(4, 2); else LAUNCH(4, 0); } \
    else if (C <= 32) MSK_TPV_LADDER(C, plan.st == 1, LAUNCH);         \
    else LAUNCH(64, 0);                                                \
  } while (0)

extern "C" {

int msk_sdf_workspace(int d, int h, int w, size_t* bytes) {
  MSK_REQUIRE(nullptr, bytes != nullptr, "bytes must not be null");
  MSK_REQUIRE(nullptr, d >= 1 && h >= 1 && w >= 1 && d <= kMaxExtent && h <= kMaxExtent && w <= kMaxExtent,
              "every extent must be in [1, 2048] (MSK_EDT_MAX_EXTENT)");
  *bytes = sdf_ws_bytes((long)d * h * w);
  return 0;
}

int msk_label_sdf(msk_ctx* ctx, const int32_t* labels, int n, int d, int h, int w, uint64_t class_mask, const double* spacing,
                  void* workspace, size_t workspace_bytes, float* phi) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, labels != nullptr && workspace != nullptr && phi != nullptr, "null labels / workspace / phi");
  MSK_REQUIRE(ctx, class_mask != 0, "class_mask must name at least one class");
  MSK_REQUIRE(ctx, boundary_count_ok(n, d, h, w),
              "every extent must be in [1, 2048] (MSK_EDT_MAX_EXTENT) and the voxel count below 2^31");
  MSK_REQUIRE(ctx, (((uintptr_t)labels) & 3) == 0, "labels must be 4-byte aligned");
  MSK_REQUIRE(ctx, (((uintptr_t)workspace) & 15) == 0 && (((uintptr_t)phi) & 15) == 0, "workspace and phi must be 16-byte aligned");
  const long V = (long)d * h * w;
  const size_t need = sdf_ws_bytes(V);
  MSK_REQUIRE(ctx, workspace_bytes >= need, "the workspace is smaller than msk_sdf_workspace asks for");
  const int nset = __builtin_popcountll(class_mask);
  const size_t phi_bytes = (size_t)n * nset * V * sizeof(float), lab_bytes = (size_t)n * V * sizeof(int32_t);
  MSK_REQUIRE(ctx, msk_bytes_disjoint(workspace, need, phi, phi_bytes) && msk_bytes_disjoint(workspace, need, labels, lab_bytes) &&
                       msk_bytes_disjoint(phi, phi_bytes, labels, lab_bytes),
              "labels, workspace and phi must not overlap");
  double* d2_out = (double*)workspace;
  double* d2_in = (double*)((char*)workspace + sdf_round256((size_t)V * sizeof(double)));
  const int nb = msk_ew_blocks(V, ctx->num_cu, 8);
  for (int s = 0; s < n; ++s) {
    const int32_t* lab = labels + (long)s * V;
    int j = 0;
    for (int c = 0; c < 64; ++c) {
      if (!((class_mask >> c) & 1)) continue;
      // (the first call checks the spacing against msk_edt3d's range before it launches anything)
      if (int rc = msk_edt_field(ctx, lab, d, h, w, c, 0, 0, spacing, d2_out)) return rc;
      if (int rc = msk_edt_field(ctx, lab, d, h, w, c, 0, 1, spacing, d2_in)) return rc;
      msk_launch_scope ls(ctx, "sdf_compose");
      hipLaunchKernelGGL(sdf_compose_k, dim3(nb), dim3(kThreads), 0, ctx->stream, lab, (const double*)d2_out, (const double*)d2_in, c,
                         V, phi + ((long)s * nset + j) * V);
      MSK_LAUNCH_CHECK(ctx);
      ++j;
    }
  }
  return 0;
}

int msk_boundary_loss_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, uint64_t class_mask,
                          const float* phi, float* out, double* stats) {
  if (boundary_check(ctx, logits, labels, class_mask, phi)) return -1;
  MSK_REQUIRE(ctx, out != nullptr && stats != nullptr, "null out / stats");
  MSK_REQUIRE(ctx, (((uintptr_t)out) & 3) == 0 && (((uintptr_t)stats) & 7) == 0, "out must be 4-byte, stats 8-byte aligned");
  const int C = logits.c;
  const BoundaryPlan plan = boundary_plan(logits, msk_quad_dense(logits), class_mask, ctx->num_cu, 3);
  const int nb = logits.n * plan.wps;
  float* partial = (float*)msk_workspace(ctx, (size_t)nb * (C + 2) * sizeof(float));
  if (!partial) return -1;
  {
    msk_launch_scope ls(ctx, "boundary_fwd_stats");
#define BOUNDARY_STATS(CM_, ST_)                                                                                                \
  hipLaunchKernelGGL((boundary_stats_k<CM_, ST_>), dim3(nb), dim3(kThreads), 0, ctx->stream, (const float*)logits.p, logits.ld, \
                     labels, phi, ignore_index, class_mask, plan.nset, plan.V, plan.wps, C, partial)
    BOUNDARY_DISPATCH(BOUNDARY_STATS);
#undef BOUNDARY_STATS
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "boundary_fwd_final");
    hipLaunchKernelGGL(boundary_final_k, dim3(1), dim3(1024), 0, ctx->stream, (const float*)partial, nb, C, plan.nset, out, stats);
    MSK_LAUNCH_CHECK(ctx);
  }
  return 0;
}

int msk_boundary_loss_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, uint64_t class_mask,
                          const float* phi, const double* stats, float coef, int accumulate, msk_tensor dlogits) {
  if (boundary_check(ctx, logits, labels, class_mask, phi)) return -1;
  const int C = logits.c;
  MSK_REQUIRE(ctx, stats != nullptr && dlogits.p != nullptr, "null stats / dlogits");
  MSK_REQUIRE(ctx, (((uintptr_t)stats) & 7) == 0 && (((uintptr_t)dlogits.p) & 3) == 0, "stats must be 8-byte, dlogits 4-byte aligned");
  MSK_REQUIRE(ctx, msk_same_shape(logits, dlogits) && dlogits.ld >= C, "dlogits shape mismatch");
  const BoundaryPlan plan = boundary_plan(logits, msk_quad_dense(logits) && msk_quad_dense(dlogits), class_mask, ctx->num_cu, 16);
  const size_t phi_bytes = (size_t)logits.n * plan.nset * plan.V * sizeof(float);
  MSK_REQUIRE(ctx, msk_bytes_disjoint(dlogits.p, tensor_bytes(dlogits), logits.p, tensor_bytes(logits)) &&
                       msk_bytes_disjoint(dlogits.p, tensor_bytes(dlogits), phi, phi_bytes),
              "dlogits must overlap neither logits nor phi");
  const int nb = logits.n * plan.wps;
  msk_launch_scope ls(ctx, "boundary_bwd");
#define BOUNDARY_BWD(CM_, ST_)                                                                                                \
  hipLaunchKernelGGL((boundary_bwd_k<CM_, ST_>), dim3(nb), dim3(kThreads), 0, ctx->stream, (const float*)logits.p, logits.ld, \
                     labels, phi, ignore_index, class_mask, plan.nset, stats, coef, accumulate, (float*)dlogits.p, dlogits.ld, \
                     plan.V, plan.wps, C)
  BOUNDARY_DISPATCH(BOUNDARY_BWD);
#undef BOUNDARY_BWD
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
