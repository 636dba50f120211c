// Top-k cross entropy (nnU-Net's TopKLoss / DC_and_topk_loss) on an exact radix SELECT: the K-th largest of n float32 values, the
// counts above and at it, and the fixed-order float64 sum above it, all on the device.  tests/topk_reference.py is the statement;
// include/msegk.h gives the record and the formulas.
//
//   order     by the sortable key of the bit pattern (sign set: all bits flipped, else the sign bit set): -0.0 < +0.0, nothing is
//             left to a float comparison.  Three digits of 11, 11 and 10 bits, most significant first (2048 bins; with 8-bit
//             digits the forward pass was one launch longer and missed its mark at two of three shapes: DESIGN.md section 7).
//   pass 1    topk_ce_k: a thread owns a voxel (the thread-per-voxel scaffold of msk_device.h, the three record forms of
//             msk_loss_region.hip), writes l = w_y (log sum exp(z - max) - (z_y - max)) or the sentinel -1 to the workspace, counts
//             the valid voxels and the first digit.  (msk_topk_select: topk_hist_k<0> over the caller's buffer instead.)
//   pass 2-3  topk_hist_k<1, 2> read the 4-byte values only and count the next digit of the keys that carry the digits found so
//             far.  No pick kernel stands between two passes: every workgroup of 256 threads rescans the global histograms of
//             the passes before it in its prologue (a thread holds 8 consecutive bins, one workgroup scan per digit:
//             topk_resolve), behind its first data load, and everything the prologue reads is asked for in one round trip.
//   sum       topk_sum_k: msk_red_chunk's lanes and tree with the predicate key > key(T) (an element outside adds +0.0), a
//             wavefront per chunk of 4096, four chunks per workgroup because the prologue wants 256 threads; a whole chunk's 16
//             quads per thread are in flight while the prologue runs.
//   finish    topk_finish_k: msk_red_finish over the chunk values, then the record and out[0] = S / K.
// K comes from the caller (select) or from n_valid and k_percent ON THE DEVICE (cross entropy); T, tie_w and 1 / K are read from
// the record by the backward kernel.  Nothing is downloaded, nothing synchronises: one 24.25 KiB memset and five launches.
// Histograms: integer LDS atomics, merged into global memory with integer atomics, one per non-empty bin and workgroup (exact, so
// the order does not matter); n_valid takes ONE global atomic per workgroup (one per wavefront, 8192 adds on one word, cost the
// first version 60 us at 2 x 96^3).  No float atomics anywhere.  The LDS adds are one atomic per lane: msk_count_slot's same-bin
// aggregation (msk_device.h; option "topk_agg_hist" 1, first digit only) was measured beside it and is 4-12 us per call slower
// at every shape of tools/bench_topk.py -- with 11-bit digits the losses of a wavefront spread over tens of bins.
// backward  reads l from the workspace (membership is the forward's, bit for bit) and recomputes only the softmax, and that only
//           in tiles of 256 voxels that hold a member; a tile without one costs label + l and a store of zeros (nothing at all
//           when the pass adds into dz).  Its first loads go out before it reads the record.
#include <cmath>

#include "msk_common.h"

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kTpvThreads, "the tpv_* helpers of msk_device.h assume this workgroup");
constexpr int kPasses = kMskSelPasses;
constexpr int kBins = kMskSelBins;
static_assert(kThreads == kMskSelThreads, "the msk_sel_* helpers of msk_device.h assume this workgroup");

struct TopkCtl {               // zeroed by one memset per call
  uint32_t hist[kPasses][kBins];
  uint32_t n_valid;            // voxels with a label in [0, C) other than ignore_index
  uint32_t pad[63];
};
static_assert(sizeof(TopkCtl) % 256 == 0, "the chunk values behind it stay aligned");

// workspace: l[n] (floats, rounded up to 256 bytes) | TopkCtl | chunk values [ceil(n / 4096)] (doubles)
struct TopkWs {
  float* loss;
  TopkCtl* ctl;
  double* partial;
};
inline size_t topk_round256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t topk_ws_bytes(long n) {
  return topk_round256((size_t)n * 4) + sizeof(TopkCtl) + topk_round256((size_t)msk_chunks_of((size_t)n) * 8);
}
inline TopkWs topk_ws(void* w, long n) {
  TopkWs s;
  s.loss = (float*)w;
  s.ctl = (TopkCtl*)((char*)w + topk_round256((size_t)n * 4));
  s.partial = (double*)((char*)s.ctl + sizeof(TopkCtl));
  return s;
}

// K -- the caller's (k_arg >= 0) or floor(n_valid * k_percent / 100), at least 1 when there is a valid voxel -- and the first NP
// digits of the K-th largest key from the global histograms of passes 0 .. NP-1 (msk_sel_load / msk_sel_scan of msk_device.h);
// K <= the number of keys.  Called by all 256 threads; s_scan: 8 LDS words.  Everything is asked for at once (one round trip).
// K == 0 returns before any barrier (uniform).
template <int NP>
__device__ __forceinline__ msk_sel topk_resolve(const TopkCtl* __restrict__ ctl, long k_arg, float kpct, uint32_t* s_scan) {
  const uint32_t* hist[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) hist[p] = ctl->hist[p];
  const msk_sel_bins<NP> bins = msk_sel_load<NP>(hist);
  const uint32_t nv = ctl->n_valid;
  uint32_t K;
  if (k_arg >= 0) {
    K = (uint32_t)k_arg;
  } else {
    K = (uint32_t)floor((double)nv * (double)kpct / 100.0);
    if (nv > 0 && K < 1) K = 1;
  }
  return msk_sel_scan<NP>(bins, K, s_scan);
}

// one value per lane into the workgroup's LDS histogram, digit < 0 = nothing; called by every lane of the wavefront
__device__ __forceinline__ void topk_count(int digit, uint32_t* __restrict__ s_hist, int lane, bool agg) {
  if (agg) {
    msk_count_slot(digit, s_hist, lane);
  } else if (digit >= 0) {
    atomicAdd(&s_hist[digit], 1u);
  }
}
// digit P of the keys whose digits 0 .. P-1 are those of the K-th largest key; grid-stride over quads (vec: x is 16-byte aligned)
// or single elements.  Every trip count is uniform over the workgroup: topk_count is reached by whole wavefronts.
template <int P>
__global__ void __launch_bounds__(kThreads)
topk_hist_k(const float* __restrict__ x, long n, int vec, TopkCtl* __restrict__ ctl, long k_arg, float kpct, int agg_on) {
  __shared__ uint32_t s_hist[kBins];
  __shared__ uint32_t s_scan[8];
  msk_sel_hist_clear(s_hist);
  const long stride = (long)gridDim.x * kThreads;
  const long n4 = n >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  // the first quad is asked for before the histograms of the passes before this one are (they cost a round trip of their own)
  long i = (long)blockIdx.x * kThreads + threadIdx.x;
  float4 cur = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec && i < n4) cur = x4[i];
  uint32_t prefix = 0u;
  if (P > 0) {
    const msk_sel sel = topk_resolve<(P > 0 ? P : 1)>(ctl, k_arg, kpct, s_scan);
    if (sel.K == 0) return;                              // uniform: the record is all zeros
    prefix = sel.prefix;
  } else {
    __syncthreads();
  }
  // same-bin aggregation (msk_count_slot) only where it is asked for and only for the first digit: behind it the digits
  // scatter and few lanes still carry the prefix
  const bool agg = P == 0 && agg_on;
  constexpr int kDigitShift = msk_sel_shift(P);
  constexpr uint32_t kDigitMask = (1u << msk_sel_width(P)) - 1u;
  auto digit_of = [&](float f) -> int {
    const uint32_t key = msk_sel_key(f);
    if (P > 0 && (key >> (kDigitShift + msk_sel_width(P))) != prefix) return -1;
    return (int)((key >> kDigitShift) & kDigitMask);
  };
  const int lane = threadIdx.x & 63;
  if (vec) {
    for (long i0 = (long)blockIdx.x * kThreads; i0 < n4; i0 += stride) {
      const bool have = i < n4;
      const float4 v = cur;
      i += stride;
      if (i < n4) cur = x4[i];                           // the next quad, ahead of the counting
      int d[4] = {-1, -1, -1, -1};
      if (have) {
        d[0] = digit_of(v.x); d[1] = digit_of(v.y); d[2] = digit_of(v.z); d[3] = digit_of(v.w);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) topk_count(d[j], s_hist, lane, agg);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {           // the last n % 4 elements
      const long e = 4 * n4 + threadIdx.x;
      topk_count(e < n ? digit_of(x[e]) : -1, s_hist, lane, agg);
    }
  } else {
    for (long i0 = (long)blockIdx.x * kThreads; i0 < n; i0 += stride) {
      const long e = i0 + threadIdx.x;
      topk_count(e < n ? digit_of(x[e]) : -1, s_hist, lane, agg);
    }
  }
  __syncthreads();
  msk_sel_hist_merge(s_hist, ctl->hist[P]);
}

// l = w_y (log sum_c exp(z_c - max) - (z_y - max)): the arithmetic of region_probs / region_stats_k at gamma = 0
template <int CM>
__device__ __forceinline__ float topk_voxel_loss(const float (&zz)[CM], int C, int y, float wy) {
  float m = -INFINITY, se = 0.f, zym = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) m = fmaxf(m, zz[c]);
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) {
      se += expf(zz[c] - m);
      if (c == y) zym = zz[c] - m;
    }
  return wy * (logf(se) - zym);
}

template <int CM, int ST>
__global__ void __launch_bounds__(kThreads)
topk_ce_k(const float* __restrict__ z, int ld, const int32_t* __restrict__ labels, const float* __restrict__ weight, int ignore_index,
          long V, int C, float* __restrict__ loss, TopkCtl* __restrict__ ctl, int agg_on) {
  __shared__ float4 tile[tpv_tile_quads(CM, ST)];
  __shared__ float s_w[64];
  __shared__ uint32_t s_hist[kBins];
  __shared__ uint32_t s_nvalid;
  msk_sel_hist_clear(s_hist);
  if (threadIdx.x == 0) s_nvalid = 0u;
  if (threadIdx.x < 64) s_w[threadIdx.x] = (weight != nullptr && (int)threadIdx.x < C) ? weight[threadIdx.x] : 1.f;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  uint32_t nvalid = 0;
  const long ntile = (V + kThreads - 1) / kThreads;
  for (long it = blockIdx.x; it < ntile; it += gridDim.x) {
    const long v0 = it * kThreads;
    const long left = V - v0;
    const int nv = (int)(left < kThreads ? left : kThreads);
    const bool mine = (int)threadIdx.x < nv;
    const long v = v0 + (mine ? threadIdx.x : 0);
    const int y = mine ? labels[v] : ignore_index;       // asked for ahead of the tile: the two latencies overlap
    tpv_fill<CM, ST>(tile, z + v0 * C, nv, C);
    const bool valid = mine && y != ignore_index && (unsigned)y < (unsigned)C;
    float l = -1.f;                                      // the sentinel of a voxel that takes no part
    if (valid) {
      float zz[CM];
      tpv_take<CM, ST>(zz, tile, z + v * ld, C);
      l = topk_voxel_loss<CM>(zz, C, y, s_w[y]);
      ++nvalid;
    }
    if (mine) loss[v] = l;
    topk_count(mine ? (int)(msk_sel_key(l) >> msk_sel_shift(0)) : -1, s_hist, lane, agg_on != 0);
  }
  nvalid = msk_wave_sum_u32(nvalid);
  if (lane == 0 && nvalid) atomicAdd(&s_nvalid, nvalid);
  __syncthreads();
  msk_sel_hist_merge(s_hist, ctl->hist[0]);
  if (threadIdx.x == 0 && s_nvalid) atomicAdd(&ctl->n_valid, s_nvalid);   // one single-word atomic per workgroup, not per wavefront
}

// msk_red_chunk's sum with a predicate, for the chunk's 64 threads (m = lane): the same loads, lanes and tree; an element whose
// key is not above tkey, or past n, adds +0.0.  The whole chunks of an aligned buffer load first (topk_chunk_load: 16 quads per
// thread, every load instruction of the wavefront 1 KiB of consecutive bytes) and add later; the others go element by element.
__device__ __forceinline__ void topk_chunk_load(const float* __restrict__ chunk0, int m, float4 (&v)[16]) {
  const float4* x4 = reinterpret_cast<const float4*>(chunk0);
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = x4[64 * j + m];
}
__device__ __forceinline__ double topk_chunk_sum_loaded(const float4 (&v)[16], uint32_t tkey) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = s[i] + (msk_sel_key(e[i]) > tkey ? (double)e[i] : 0.0);
  }
  return msk_red_chunk_tree(s);
}
__device__ __forceinline__ double topk_chunk_sum_ragged(const float* __restrict__ xc, long left, int m, uint32_t tkey) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < 16; ++j) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long e = 256L * j + 4 * m + i;
      double d = 0.0;
      if (e < left) {
        const float f = xc[e];
        if (msk_sel_key(f) > tkey) d = (double)f;
      }
      s[i] = s[i] + d;
    }
  }
  return msk_red_chunk_tree(s);
}

constexpr int kSumChunks = kThreads / 64;                // chunks per workgroup of topk_sum_k

__global__ void __launch_bounds__(kThreads)
topk_sum_k(const float* __restrict__ x, long n, int vec, long nc, const TopkCtl* __restrict__ ctl, long k_arg, float kpct,
           double* __restrict__ partial) {
  __shared__ uint32_t s_scan[8];
  const int m = threadIdx.x & 63;
  const long chunk = (long)blockIdx.x * kSumChunks + (threadIdx.x >> 6);
  const long base = chunk * kMskRedChunk;
  const bool active = chunk < nc;                        // uniform over a wavefront
  const bool whole = active && vec && n - base >= kMskRedChunk;
  float4 v[16];
  if (whole) topk_chunk_load(x + base, m, v);            // in flight while the histograms are read and scanned
  const msk_sel sel = topk_resolve<kPasses>(ctl, k_arg, kpct, s_scan);
  if (sel.K == 0) return;                                // uniform; the finish pass does not read the chunk values then
  const uint32_t tkey = sel.prefix;
  if (!active) return;                                   // behind the last barrier
  const double s = whole ? topk_chunk_sum_loaded(v, tkey) : topk_chunk_sum_ragged(x + base, n - base, m, tkey);
  if (m == 0) partial[chunk] = s;
}

// one workgroup of 256.  rec = {T, K, n_gt, n_eq, S_gt, r, tie_w, S}; out (nullable): {S / K, 0, 0 x C}
__global__ void __launch_bounds__(kMskRedLanes)
topk_finish_k(long nc, const TopkCtl* __restrict__ ctl, long k_arg, float kpct, const double* __restrict__ partial,
              double* __restrict__ rec, float* __restrict__ out, int C) {
  __shared__ uint32_t s_scan[8];
  const msk_sel sel = topk_resolve<kPasses>(ctl, k_arg, kpct, s_scan);
  const uint32_t K = sel.K;
  if (out != nullptr && (int)threadIdx.x >= 1 && (int)threadIdx.x < 2 + C) out[threadIdx.x] = 0.f;
  if (K == 0) {
    if (threadIdx.x < 8) rec[threadIdx.x] = 0.0;
    if (out != nullptr && threadIdx.x == 0) out[0] = 0.f;
    return;
  }
  const msk_red_vals red = msk_red_finish<false>(nc, nullptr, partial, nullptr, nullptr);
  if (threadIdx.x == 0) {
    const double T = (double)msk_sel_unkey(sel.prefix);
    const double r = (double)(K - sel.ngt);              // >= 1: fewer than K keys are above the K-th largest
    const double S = __dadd_rn(red.sumsq, __dmul_rn(r, T));   // two roundings, as the statement has them
    rec[0] = T;
    rec[1] = (double)K;
    rec[2] = (double)sel.ngt;
    rec[3] = (double)sel.neq;
    rec[4] = red.sumsq;
    rec[5] = r;
    rec[6] = r / (double)sel.neq;
    rec[7] = S;
    if (out != nullptr) out[0] = (float)(S / (double)K);
  }
}

// dz (+)= coef u w_y (softmax(z) - onehot(y)) / K, u = 1 above T, tie_w at T, 0 below and at a voxel that took no part
template <int CM, int ST>
__global__ void __launch_bounds__(kThreads)
topk_bwd_k(const float* __restrict__ z, int ld, const int32_t* __restrict__ labels, const float* __restrict__ weight, int ignore_index,
           const float* __restrict__ loss, const double* __restrict__ rec, float coef, int accumulate, float* __restrict__ dz,
           int lddz, long V, int C) {
  __shared__ float4 tile[tpv_tile_quads(CM, ST)];
  __shared__ float s_w[64];
  const long ntile = (V + kThreads - 1) / kThreads;
  long it = blockIdx.x;                                  // < ntile: the grid is no larger
  // the first tile's label and l are asked for before the record is (it is the forward's last store)
  int y = ignore_index;
  float lv = -1.f;
  if (it * kThreads + threadIdx.x < V) {
    y = labels[it * kThreads + threadIdx.x];
    lv = loss[it * kThreads + threadIdx.x];
  }
  if (threadIdx.x < 64) s_w[threadIdx.x] = (weight != nullptr && (int)threadIdx.x < C) ? weight[threadIdx.x] : 1.f;
  const double Kd = rec[1];
  const uint32_t tkey = msk_sel_key((float)rec[0]);
  const float tie = (float)rec[6];
  const float scale = Kd > 0.0 ? (float)((double)coef / Kd) : 0.f;
  __syncthreads();
  for (; it < ntile; it += gridDim.x) {
    const long v0 = it * kThreads;
    const long left = V - v0;
    const int nv = (int)(left < kThreads ? left : kThreads);
    const bool mine = (int)threadIdx.x < nv;
    const long v = v0 + (mine ? threadIdx.x : 0);
    const bool valid = mine && y != ignore_index && (unsigned)y < (unsigned)C;
    float u = 0.f;
    if (valid && Kd > 0.0) {
      const uint32_t key = msk_sel_key(lv);
      u = key > tkey ? 1.f : (key == tkey ? tie : 0.f);
    }
    const int yv = y;
    const long nx = (it + gridDim.x) * kThreads + threadIdx.x;   // the next tile's voxel
    if (it + gridDim.x < ntile && nx < V) {
      y = labels[nx];
      lv = loss[nx];
    } else {
      y = ignore_index;
    }
    if (!__syncthreads_or(u != 0.f)) {                   // no member in this tile: the gradient is exactly 0
      if (!accumulate) {
        if (ST) {
          float* dt = dz + v0 * C;                       // dense, 16-byte aligned: v0 is a multiple of 256
          const int nf = nv * C, nq = nf >> 2;
          for (int i = threadIdx.x; i < nq; i += kThreads) reinterpret_cast<float4*>(dt)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          for (int i = 4 * nq + threadIdx.x; i < nf; i += kThreads) dt[i] = 0.f;
        } else if (mine) {
          float* dp = dz + v * lddz;
          for (int c = 0; c < C; ++c) dp[c] = 0.f;
        }
      }
      continue;                                          // uniform over the workgroup
    }
    tpv_fill<CM, ST>(tile, z + v0 * C, nv, C);
    float zz[CM];
    if (u != 0.f) {
      tpv_take<CM, ST>(zz, tile, z + v * ld, C);
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
      const float f = scale * u * s_w[yv];
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) zz[c] = f * (zz[c] * inv - (c == yv ? 1.f : 0.f));
    } else {
#pragma unroll
      for (int c = 0; c < CM; ++c) zz[c] = 0.f;
    }
    if (ST) {
      tpv_put<CM, ST>(zz, tile, dz + v0 * C, C, nv, mine, accumulate != 0);
    } else if (mine) {
      float* dp = dz + v * lddz;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) dp[c] = accumulate ? dp[c] + zz[c] : zz[c];
    }
  }
}

// the record form of a call: 2 = flat LDS tile (dense, C <= 4), 1 = quad tile (dense, C % 4 == 0, C <= 32), 0 = a lane's own
inline int topk_form(int C, bool dense) { return !dense ? 0 : (C <= 4 ? 2 : ((C % 4 == 0 && C <= 32) ? 1 : 0)); }

int topk_ce_check(msk_ctx* ctx, const msk_tensor& logits, const int32_t* labels, const float* weights, const void* workspace,
                  const double* record) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, logits.p != nullptr && labels != nullptr && workspace != nullptr && record != nullptr,
              "null logits / labels / workspace / record");
  MSK_REQUIRE(ctx, logits.c >= 2 && logits.c <= 64, "num_classes must be in [2,64]");
  MSK_REQUIRE(ctx, logits.ld >= logits.c, "logits.ld must be >= logits.c");
  MSK_REQUIRE(ctx, logits.n >= 1 && logits.d >= 1 && logits.h >= 1 && logits.w >= 1 && msk_voxels(logits) <= 0x7fffffffL,
              "voxel count must be in [1, 2^31)");
  MSK_REQUIRE(ctx, ((((uintptr_t)logits.p) | ((uintptr_t)labels) | ((uintptr_t)weights)) & 3) == 0,
              "logits / labels / weights must be 4-byte aligned");
  MSK_REQUIRE(ctx, (((uintptr_t)workspace) & 15) == 0 && (((uintptr_t)record) & 7) == 0,
              "workspace must be 16-byte, record 8-byte aligned");
  const long V = msk_voxels(logits);
  const size_t wb = topk_ws_bytes(V);
  MSK_REQUIRE(ctx, msk_bytes_disjoint(workspace, wb, logits.p, ((size_t)(V - 1) * logits.ld + logits.c) * 4) &&
                       msk_bytes_disjoint(workspace, wb, labels, (size_t)V * 4) && msk_bytes_disjoint(workspace, wb, record, 64) &&
                       (weights == nullptr || msk_bytes_disjoint(workspace, wb, weights, (size_t)logits.c * 4)),
              "workspace overlaps an operand");
  return 0;
}

// passes 2 and 3, the sum and the finish over the n values of x, whose first digits topk_ce_k or topk_hist_k<0> counted
int topk_tail(msk_ctx* ctx, const float* x, long n, const TopkWs& ws, long k_arg, float kpct, double* record, float* out, int C) {
  const int vec = (((uintptr_t)x) & 15) == 0;
  const int nb = msk_ew_blocks(vec ? (n + 3) / 4 : n, ctx->num_cu, 2);
  const int agg = ctx->topk_agg_hist;
  {
    msk_launch_scope ls(ctx, "topk_hist");
    hipLaunchKernelGGL((topk_hist_k<1>), dim3(nb), dim3(kThreads), 0, ctx->stream, x, n, vec, ws.ctl, k_arg, kpct, agg);
    hipLaunchKernelGGL((topk_hist_k<2>), dim3(nb), dim3(kThreads), 0, ctx->stream, x, n, vec, ws.ctl, k_arg, kpct, agg);
    MSK_LAUNCH_CHECK(ctx);
  }
  const long nc = msk_chunks_of((size_t)n);
  {
    msk_launch_scope ls(ctx, "topk_sum");
    hipLaunchKernelGGL(topk_sum_k, dim3((unsigned)((nc + kSumChunks - 1) / kSumChunks)), dim3(kThreads), 0, ctx->stream, x, n, vec,
                       nc, (const TopkCtl*)ws.ctl, k_arg, kpct, ws.partial);
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "topk_finish");
    hipLaunchKernelGGL(topk_finish_k, dim3(1), dim3(kMskRedLanes), 0, ctx->stream, nc, (const TopkCtl*)ws.ctl, k_arg, kpct,
                       (const double*)ws.partial, record, out, C);
    MSK_LAUNCH_CHECK(ctx);
  }
  return 0;
}

}  // namespace

// CM: register arrays sized to the class count in steps of a quad, as the region kernels do; 33..64 classes take the lane's-own
// form only
#define TOPK_DISPATCH(LAUNCH)                                   \
  do {                                                          \
    if (C <= 4) { if (st == 2) LAUNCH(4, 2); else LAUNCH(4, 0); } \
    else if (C <= 32) MSK_TPV_LADDER(C, st == 1, LAUNCH);       \
    else LAUNCH(64, 0);                                         \
  } while (0)

extern "C" {

int msk_topk_workspace(long n, size_t* bytes) {
  MSK_REQUIRE(nullptr, bytes != nullptr, "bytes must not be null");
  MSK_REQUIRE(nullptr, n >= 1 && n <= 0x7fffffffL, "n must be in [1, 2^31)");
  *bytes = topk_ws_bytes(n);
  return 0;
}

int msk_topk_select(msk_ctx* ctx, const float* x, long n, long k, void* workspace, double* record) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, x != nullptr && workspace != nullptr && record != nullptr, "null x / workspace / record");
  MSK_REQUIRE(ctx, n >= 1 && n <= 0x7fffffffL, "n must be in [1, 2^31)");
  MSK_REQUIRE(ctx, k >= 0 && k <= n, "k must be in [0, n]");
  MSK_REQUIRE(ctx, (((uintptr_t)x) & 3) == 0, "x must be 4-byte aligned");
  MSK_REQUIRE(ctx, (((uintptr_t)workspace) & 15) == 0 && (((uintptr_t)record) & 7) == 0,
              "workspace must be 16-byte, record 8-byte aligned");
  const size_t wb = topk_ws_bytes(n);
  MSK_REQUIRE(ctx, msk_bytes_disjoint(workspace, wb, x, (size_t)n * 4) && msk_bytes_disjoint(workspace, wb, record, 64),
              "workspace overlaps an operand");
  const TopkWs ws = topk_ws(workspace, n);
  MSK_CHECK_HIP(ctx, hipMemsetAsync(ws.ctl, 0, sizeof(TopkCtl), ctx->stream));
  const int vec = (((uintptr_t)x) & 15) == 0;
  {
    msk_launch_scope ls(ctx, "topk_hist0");
    hipLaunchKernelGGL((topk_hist_k<0>), dim3(msk_ew_blocks(vec ? (n + 3) / 4 : n, ctx->num_cu, 2)), dim3(kThreads), 0, ctx->stream,
                       x, n, vec, ws.ctl, k, 0.f, ctx->topk_agg_hist);
    MSK_LAUNCH_CHECK(ctx);
  }
  return topk_tail(ctx, x, n, ws, k, 0.f, record, nullptr, 0);
}

int msk_topk_ce_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, const float* weights, float k_percent,
                    void* workspace, float* out, double* record) {
  if (topk_ce_check(ctx, logits, labels, weights, workspace, record)) return -1;
  MSK_REQUIRE(ctx, out != nullptr && (((uintptr_t)out) & 3) == 0, "out must be a 4-byte aligned pointer");
  MSK_REQUIRE(ctx, k_percent > 0.f && k_percent <= 100.f, "k_percent must be in (0, 100]");
  const int C = logits.c;
  const long V = msk_voxels(logits);
  MSK_REQUIRE(ctx, msk_bytes_disjoint(workspace, topk_ws_bytes(V), out, (size_t)(2 + C) * 4), "workspace overlaps an operand");
  const TopkWs ws = topk_ws(workspace, V);
  MSK_CHECK_HIP(ctx, hipMemsetAsync(ws.ctl, 0, sizeof(TopkCtl), ctx->stream));
  const int st = topk_form(C, msk_quad_dense(logits));
  const int nb = msk_ew_blocks(V, ctx->num_cu, 4);
  const int agg = ctx->topk_agg_hist;
  {
    msk_launch_scope ls(ctx, "topk_ce_fwd");
#define TOPK_CE(CM_, ST_)                                                                                                    \
  hipLaunchKernelGGL((topk_ce_k<CM_, ST_>), dim3(nb), dim3(kThreads), 0, ctx->stream, (const float*)logits.p, logits.ld, labels, \
                     weights, ignore_index, V, C, ws.loss, ws.ctl, agg)
    TOPK_DISPATCH(TOPK_CE);
#undef TOPK_CE
    MSK_LAUNCH_CHECK(ctx);
  }
  return topk_tail(ctx, ws.loss, V, ws, -1, k_percent, record, out, C);
}

int msk_topk_ce_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, const float* weights,
                    const void* workspace, const double* record, float coef, int accumulate, msk_tensor dz) {
  if (topk_ce_check(ctx, logits, labels, weights, workspace, record)) return -1;
  const int C = logits.c;
  const long V = msk_voxels(logits);
  MSK_REQUIRE(ctx, dz.p != nullptr && (((uintptr_t)dz.p) & 3) == 0, "dz must be a 4-byte aligned pointer");
  MSK_REQUIRE(ctx, msk_same_shape(logits, dz) && dz.ld >= C, "dz shape mismatch");
  MSK_REQUIRE(ctx, msk_bytes_disjoint(workspace, topk_ws_bytes(V), dz.p, ((size_t)(V - 1) * dz.ld + C) * 4),
              "workspace overlaps an operand");
  const TopkWs ws = topk_ws(const_cast<void*>(workspace), V);
  const int st = topk_form(C, msk_quad_dense(logits) && msk_quad_dense(dz));
  const int nb = msk_ew_blocks(V, ctx->num_cu, 16);
  msk_launch_scope ls(ctx, "topk_ce_bwd");
#define TOPK_BWD(CM_, ST_)                                                                                                    \
  hipLaunchKernelGGL((topk_bwd_k<CM_, ST_>), dim3(nb), dim3(kThreads), 0, ctx->stream, (const float*)logits.p, logits.ld, labels, \
                     weights, ignore_index, (const float*)ws.loss, record, coef, accumulate, (float*)dz.p, dz.ld, V, C)
  TOPK_DISPATCH(TOPK_BWD);
#undef TOPK_BWD
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
