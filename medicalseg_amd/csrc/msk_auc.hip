// Exact one-vs-rest ROC-AUC counts of softmax scores against a label, per class three integers {U2, n_pos, n_neg}:
//   U2 = sum over positives i of ( 2 * #{negatives j : s_j < s_i} + #{negatives j : s_j == s_i} ),
// so AUC = U2 / (2 * n_pos * n_neg) (Mann-Whitney with average ranks for ties = what sklearn's roc_auc_score integrates;
// reference core/val.py:121-131,174 and utils/metric.py:64-107).  Integers only: the result does not depend on the schedule.
//
// Three stages.
//   pack   (msk_auc_pack): per class one 32-bit key per voxel, bits 0-30 = the bits of the non-negative float score (already in
//          float order), bit 31 = "label == class".  Rows of C scores go through an LDS tile (16-byte global loads, padded pitch);
//          each of the C key streams is written one word per lane, coalesced.
//   sort   (msk_auc_counts): LSD radix sort on bits 0-30, four 8-bit digit passes (the last has 7 bits), ping-pong between the key
//          buffer and a scratch buffer.  A pass is histogram -> exclusive scan -> stable scatter over chunks of kChunk keys; the
//          scan is two kernels (tiles of kScanTile entries, then the tile sums), so no workgroup waits for another: every
//          dependency between workgroups is a kernel boundary.  All classes in one launch (gridDim.y).
//   count  on the sorted keys, N(p) = negatives at positions < p; a positive in the run of equal scores [a, b) adds
//          2 N(a) + (N(b) - N(a)) = N(a) + N(b).  auc_blocks_k: per chunk the negatives, and the local N at its first and last
//          run head; auc_carry_k (one workgroup per class): prefix sum of the negatives, forward max-scan of the last-head values
//          and backward min-scan of the first-head values over the chunks (N is non-decreasing, so the latest head before a
//          position has the largest N and the next head behind it the smallest); auc_sum_k: the same scans inside a chunk and one
//          64-bit atomic per workgroup.  A run may span any number of chunks; nothing is serial per run.
#include "msk_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kIpt = 16;                    // keys per thread
constexpr int kChunk = kThreads * kIpt;     // keys per workgroup
constexpr int kScanThreads = 1024;
constexpr int kScanTile = 4 * kScanThreads; // histogram entries per workgroup of the first scan kernel
constexpr uint32_t kScoreMask = 0x7fffffffu;
constexpr uint32_t kNone = 0xffffffffu;

// ---- pack ----------------------------------------------------------------------------------------------------
// grid-stride over tiles of tv voxels; dynamic LDS: tv * (C | 1) words
__global__ void __launch_bounds__(kThreads)
auc_pack_k(const float* __restrict__ x, int ld, long voxels, int C, const int32_t* __restrict__ label,
           uint32_t* __restrict__ keys, long capacity, long offset, int tv, unsigned long long* __restrict__ status) {
  extern __shared__ uint32_t tile[];
  const int P = C | 1;
  const int t = threadIdx.x;
  const bool dense = ld == C && (((uintptr_t)x) & 15) == 0;   // tv * C is a multiple of 4: every tile starts on 16 bytes
  const long ntiles = (voxels + tv - 1) / tv;
  unsigned bad_label = 0, bad_score = 0;
  for (long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const long v0 = tl * tv;
    const int nv = (int)(voxels - v0 < tv ? voxels - v0 : tv);
    const int words = nv * C;
    if (dense) {
      const uint4* s4 = reinterpret_cast<const uint4*>(x + v0 * C);
      for (int q = t; q < words / 4; q += kThreads) {
        const uint4 r = s4[q];
        int v = (4 * q) / C, c = 4 * q - v * C;
        const uint32_t e[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          tile[v * P + c] = e[j];
          if (++c == C) { c = 0; ++v; }
        }
      }
      for (int i = (words & ~3) + t; i < words; i += kThreads) {   // the last tile of a volume whose nv * C is not a multiple of 4
        const int v = i / C, c = i - v * C;
        tile[v * P + c] = __float_as_uint(x[v0 * C + i]);
      }
    } else {
      for (int i = t; i < words; i += kThreads) {
        const int v = i / C, c = i - v * C;
        tile[v * P + c] = __float_as_uint(x[(v0 + v) * ld + c]);
      }
    }
    __syncthreads();
    for (int v = t; v < nv; v += kThreads) {
      const int lab = label[v0 + v];
      if ((unsigned)lab >= (unsigned)C) ++bad_label;
      uint32_t* dst = keys + offset + v0 + v;
      for (int c = 0; c < C; ++c) {
        uint32_t u = tile[v * P + c];
        if (u == 0x80000000u) u = 0;   // -0.0 == +0.0
        if ((u & 0x80000000u) || (u & 0x7f800000u) == 0x7f800000u) ++bad_score;   // negative, infinite or NaN
        dst[(size_t)c * (size_t)capacity] = (u & kScoreMask) | (lab == c ? 0x80000000u : 0u);
      }
    }
    __syncthreads();
  }
  // one atomic per wavefront and word, only where something was found
  for (int o = 32; o > 0; o >>= 1) {
    bad_label += __shfl_down(bad_label, o, 64);
    bad_score += __shfl_down(bad_score, o, 64);
  }
  if ((t & 63) == 0) {
    if (bad_label) atomicAdd(&status[0], (unsigned long long)bad_label);
    if (bad_score) atomicAdd(&status[1], (unsigned long long)bad_score);
  }
}

// ---- sort: one digit pass ---------------------------------------------------------------------------------------
// hist[class][digit * nb + chunk], nb = chunks of a class
__global__ void __launch_bounds__(kThreads)
auc_hist_k(const uint32_t* __restrict__ in, size_t in_stride, int count, int nb, int shift, uint32_t mask,
           uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const uint32_t* kc = in + (size_t)blockIdx.y * in_stride;
  h[threadIdx.x] = 0;
  const long beg = (long)blockIdx.x * kChunk;
  uint32_t key[kIpt];
#pragma unroll
  for (int r = 0; r < kIpt; ++r) {
    const long i = beg + r * kThreads + (long)threadIdx.x;
    key[r] = i < count ? kc[i] : 0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kIpt; ++r)
    if (beg + r * kThreads + (long)threadIdx.x < count) atomicAdd(&h[(key[r] >> shift) & mask], 1u);
  __syncthreads();
  hist[(size_t)blockIdx.y * 256 * nb + (size_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan inside every tile of kScanTile entries; the tile's sum goes to part[class][tile]
__global__ void __launch_bounds__(kScanThreads)
auc_scan_tiles_k(uint32_t* __restrict__ hist, int total, int npart, uint32_t* __restrict__ part) {
  __shared__ uint32_t wtot[kScanThreads / 64];
  uint32_t* h = hist + (size_t)blockIdx.y * total;
  const int base = blockIdx.x * kScanTile + threadIdx.x * 4;
  uint32_t v[4], s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = base + j < total ? h[base + j] : 0;
    s += v[j];
  }
  uint32_t all;
  uint32_t run = msk_block_excl_scan<false>(s, 0u, msk_op_add(), wtot, &all);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (base + j < total) h[base + j] = run;
    run += v[j];
  }
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * npart + blockIdx.x] = all;
}

// exclusive scan of the npart tile sums of a class, one workgroup per class
__global__ void __launch_bounds__(kScanThreads)
auc_scan_parts_k(uint32_t* __restrict__ part, int npart) {
  __shared__ uint32_t wtot[kScanThreads / 64];
  uint32_t* p = part + (size_t)blockIdx.y * npart;
  uint32_t carry = 0;
  for (int base = 0; base < npart; base += kScanThreads) {
    const int i = base + threadIdx.x;
    const uint32_t v = i < npart ? p[i] : 0;
    uint32_t all;
    const uint32_t ex = msk_block_excl_scan<false>(v, 0u, msk_op_add(), wtot, &all);
    if (i < npart) p[i] = carry + ex;
    carry += all;
  }
}

// stable scatter: rounds of 256 keys in order; a lane's place among the equal digits of its wavefront comes from eight ballots,
// the wavefronts before it from LDS counts, the rounds before it from a running offset per digit
__global__ void __launch_bounds__(kThreads)
auc_scatter_k(const uint32_t* __restrict__ in, size_t in_stride, uint32_t* __restrict__ out, size_t out_stride, int count,
              int nb, int npart, int shift, uint32_t mask, const uint32_t* __restrict__ hist, const uint32_t* __restrict__ part) {
  constexpr int NW = kThreads / 64;
  __shared__ uint32_t run[256];
  __shared__ uint32_t wcnt[NW][256];
  const uint32_t* kc = in + (size_t)blockIdx.y * in_stride;
  uint32_t* oc = out + (size_t)blockIdx.y * out_stride;
  const uint32_t* hc = hist + (size_t)blockIdx.y * 256 * nb;
  const uint32_t* pc = part + (size_t)blockIdx.y * npart;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {
    const int e = tid * nb + (int)blockIdx.x;
    run[tid] = hc[e] + pc[e / kScanTile];
  }
  const unsigned long long lt = (1ull << lane) - 1ull;
  const long beg = (long)blockIdx.x * kChunk;
  uint32_t key[kIpt];
#pragma unroll
  for (int r = 0; r < kIpt; ++r) {
    const long i = beg + r * kThreads + tid;
    key[r] = i < count ? kc[i] : 0;
  }
#pragma unroll
  for (int r = 0; r < kIpt; ++r) {
    if (beg + r * kThreads >= count) break;   // uniform over the workgroup
    for (int i = tid; i < NW * 256; i += kThreads) (&wcnt[0][0])[i] = 0;
    __syncthreads();
    const bool valid = beg + r * kThreads + tid < count;
    const int dg = (int)((key[r] >> shift) & mask);
    unsigned long long match = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long bb = __ballot((dg >> b) & 1);
      match &= ((dg >> b) & 1) ? bb : ~bb;
    }
    const int pre = __popcll(match & lt);
    if (valid && pre == 0) wcnt[wave][dg] = (uint32_t)__popcll(match);
    __syncthreads();
    if (valid) {
      uint32_t pos = run[dg] + (uint32_t)pre;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][dg];
      if (pos < (uint32_t)count) oc[pos] = key[r];   // always true for a correct histogram: a guard, not a case
    }
    __syncthreads();
    {
      uint32_t s = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) s += wcnt[w][tid];
      run[tid] += s;
    }
    __syncthreads();
  }
}

// ---- count ---------------------------------------------------------------------------------------------------
// A thread's kIpt CONSECUTIVE sorted keys as three bit masks: negative, positive, run head (score differs from the key on
// its left, which is read from global memory whatever workgroup owns it).  q = position of the thread's first key.
__device__ __forceinline__ void load_flags(const uint32_t* __restrict__ kc, long count, long q, uint32_t& negm, uint32_t& posm,
                                           uint32_t& headm) {
  uint32_t k[kIpt];
  if (q + kIpt <= count && (((uintptr_t)kc) & 15) == 0) {
    const uint4* k4 = reinterpret_cast<const uint4*>(kc + q);
#pragma unroll
    for (int j = 0; j < kIpt / 4; ++j) {
      const uint4 r = k4[j];
      k[4 * j] = r.x; k[4 * j + 1] = r.y; k[4 * j + 2] = r.z; k[4 * j + 3] = r.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kIpt; ++j) k[j] = q + j < count ? kc[q + j] : 0;
  }
  uint32_t prev = (q > 0 && q < count) ? kc[q - 1] : 0;
  negm = posm = headm = 0;
#pragma unroll
  for (int j = 0; j < kIpt; ++j) {
    if (q + j < count) {
      if (k[j] >> 31) posm |= 1u << j; else negm |= 1u << j;
      if (q + j == 0 || ((k[j] ^ prev) & kScoreMask) != 0) headm |= 1u << j;
    }
    prev = k[j];
  }
}

__device__ __forceinline__ uint32_t below(uint32_t m, int j) { return (uint32_t)__popc(m & ((1u << j) - 1u)); }

// per chunk: blk[0][chunk] = negatives, blk[1][chunk] = 1 + local N at the last run head (0 = the chunk has no head),
// blk[2][chunk] = local N at the first run head (kNone = no head); local N = negatives of the chunk in front of the position
__global__ void __launch_bounds__(kThreads)
auc_blocks_k(const uint32_t* __restrict__ keys, size_t stride, int count, int nb, uint32_t* __restrict__ blk) {
  __shared__ uint32_t wtot[kThreads / 64];
  const uint32_t* kc = keys + (size_t)blockIdx.y * stride;
  uint32_t negm, posm, headm;
  load_flags(kc, count, (long)blockIdx.x * kChunk + (long)threadIdx.x * kIpt, negm, posm, headm);
  uint32_t nneg;
  const uint32_t ex = msk_block_excl_scan<false>((uint32_t)__popc(negm), 0u, msk_op_add(), wtot, &nneg);
  const uint32_t last = headm ? ex + below(negm, 31 - __clz((int)headm)) + 1u : 0u;
  const uint32_t first = headm ? ex + below(negm, __ffs((int)headm) - 1) : kNone;
  uint32_t lastmax, firstmin;
  msk_block_excl_scan<false>(last, 0u, msk_op_max(), wtot, &lastmax);
  msk_block_excl_scan<false>(first, kNone, msk_op_min(), wtot, &firstmin);
  if (threadIdx.x == 0) {
    uint32_t* b = blk + (size_t)blockIdx.y * 3 * nb;
    b[blockIdx.x] = nneg;
    b[nb + blockIdx.x] = lastmax;
    b[2 * nb + blockIdx.x] = firstmin;
  }
}

// One workgroup per class over the nb chunk records, a thread owning a contiguous segment of them.  In place:
// blk[0] -> negatives in front of the chunk, blk[1] -> N(a) of the run that enters the chunk (the last head in front of it),
// blk[2] -> N at the first head behind the chunk (n_neg when there is none).  Also out[class] = {0, n_pos, n_neg}.
__global__ void __launch_bounds__(kScanThreads)
auc_carry_k(uint32_t* __restrict__ blk, int nb, int count, unsigned long long* __restrict__ out) {
  __shared__ uint32_t wtot[kScanThreads / 64];
  uint32_t* base = blk + (size_t)blockIdx.y * 3 * nb;
  uint32_t* lastv = base + nb;
  uint32_t* firstv = base + 2 * nb;
  const int seg = (nb + kScanThreads - 1) / kScanThreads;
  const int b0 = min(nb, (int)threadIdx.x * seg), b1 = min(nb, b0 + seg);
  uint32_t s = 0;
  for (int b = b0; b < b1; ++b) s += base[b];
  uint32_t nneg;
  uint32_t run = msk_block_excl_scan<false>(s, 0u, msk_op_add(), wtot, &nneg);
  uint32_t segmax = 0, segmin = kNone;
  for (int b = b0; b < b1; ++b) {   // local head values -> values of N
    const uint32_t n = base[b], l = lastv[b], f = firstv[b];
    base[b] = run;
    if (l) {
      lastv[b] = run + l - 1u;
      firstv[b] = run + f;
      segmax = lastv[b];                       // N is non-decreasing: the latest head has the largest value ...
      if (segmin == kNone) segmin = firstv[b]; // ... and the earliest the smallest
    } else {
      lastv[b] = 0;
      firstv[b] = kNone;
    }
    run += n;
  }
  uint32_t all;
  uint32_t fwd = msk_block_excl_scan<false>(segmax, 0u, msk_op_max(), wtot, &all);
  uint32_t bwd = msk_block_excl_scan<true>(segmin, kNone, msk_op_min(), wtot, &all);
  for (int b = b0; b < b1; ++b) {
    const uint32_t l = lastv[b];
    lastv[b] = fwd;
    fwd = fwd > l ? fwd : l;
  }
  for (int b = b1 - 1; b >= b0; --b) {
    const uint32_t f = firstv[b];
    firstv[b] = bwd == kNone ? nneg : bwd;
    bwd = bwd < f ? bwd : f;
  }
  if (threadIdx.x == 0) {
    unsigned long long* o = out + (size_t)blockIdx.y * 3;
    o[0] = 0;
    o[1] = (unsigned long long)((uint32_t)count - nneg);
    o[2] = (unsigned long long)nneg;
  }
}

__global__ void __launch_bounds__(kThreads)
auc_sum_k(const uint32_t* __restrict__ keys, size_t stride, int count, int nb, const uint32_t* __restrict__ blk,
          unsigned long long* __restrict__ out) {
  __shared__ uint32_t wtot[kThreads / 64];
  __shared__ unsigned long long wsum[kThreads / 64];
  const uint32_t* kc = keys + (size_t)blockIdx.y * stride;
  const uint32_t* b = blk + (size_t)blockIdx.y * 3 * nb;
  uint32_t negm, posm, headm;
  load_flags(kc, count, (long)blockIdx.x * kChunk + (long)threadIdx.x * kIpt, negm, posm, headm);
  uint32_t all;
  const uint32_t n0 = b[blockIdx.x] + msk_block_excl_scan<false>((uint32_t)__popc(negm), 0u, msk_op_add(), wtot, &all);   // N of the thread's first key
  const uint32_t last = headm ? n0 + below(negm, 31 - __clz((int)headm)) : 0u;
  const uint32_t first = headm ? n0 + below(negm, __ffs((int)headm) - 1) : kNone;
  uint32_t na = msk_block_excl_scan<false>(last, 0u, msk_op_max(), wtot, &all);
  uint32_t nbk = msk_block_excl_scan<true>(first, kNone, msk_op_min(), wtot, &all);
  const uint32_t cin = b[nb + blockIdx.x], cout = b[2 * nb + blockIdx.x];
  na = na > cin ? na : cin;
  nbk = nbk < cout ? nbk : cout;
  // N(b) of every key: the value at the next head behind it, walking backwards
  uint32_t nbv[kIpt];
#pragma unroll
  for (int j = kIpt - 1; j >= 0; --j) {
    nbv[j] = nbk;
    if ((headm >> j) & 1) nbk = n0 + below(negm, j);
  }
  unsigned long long sum = 0;
#pragma unroll
  for (int j = 0; j < kIpt; ++j) {
    if ((headm >> j) & 1) na = n0 + below(negm, j);
    if ((posm >> j) & 1) sum += (unsigned long long)na + (unsigned long long)nbv[j];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < kThreads / 64; ++w) s += wsum[w];
    if (s) atomicAdd(&out[(size_t)blockIdx.y * 3], s);
  }
}

// workspace layout of msk_auc_counts, every part on a 256-byte boundary
struct AucLayout {
  size_t stride;    // scratch keys per class
  int nb, npart;
  size_t scratch, hist, part, blk, total;   // byte offsets
};

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

inline AucLayout auc_layout(long count, int classes) {
  AucLayout L;
  L.stride = ((size_t)count + 3) & ~(size_t)3;
  L.nb = (int)((count + kChunk - 1) / kChunk);
  L.npart = (int)(((long)256 * L.nb + kScanTile - 1) / kScanTile);
  L.scratch = 0;
  L.hist = up256(L.scratch + (size_t)classes * L.stride * 4);
  L.part = up256(L.hist + (size_t)classes * 256 * L.nb * 4);
  L.blk = up256(L.part + (size_t)classes * L.npart * 4);
  L.total = up256(L.blk + (size_t)classes * 3 * L.nb * 4);
  return L;
}

}  // namespace

extern "C" {

int msk_auc_pack(msk_ctx* ctx, msk_tensor probs, const int32_t* label, uint32_t* keys, long capacity, long offset,
                 unsigned long long* status) {
  const int C = probs.c;
  const long voxels = msk_voxels(probs);
  MSK_REQUIRE(ctx, C >= 1 && C <= 64, "classes (probs.c) must be in [1,64]");
  MSK_REQUIRE(ctx, probs.p != nullptr && label != nullptr && keys != nullptr && status != nullptr, "null probs / label / keys / status");
  MSK_REQUIRE(ctx, probs.ld >= C, "probs.ld < probs.c");
  MSK_REQUIRE(ctx, voxels >= 1, "empty probs");
  MSK_REQUIRE(ctx, offset >= 0 && capacity >= 1 && offset + voxels <= capacity, "offset + voxels exceeds capacity");
  MSK_REQUIRE(ctx, capacity <= 0x7fffffffL, "capacity must be below 2^31 keys per class");
  MSK_REQUIRE(ctx, ((((uintptr_t)probs.p) | ((uintptr_t)label) | ((uintptr_t)keys)) & 3) == 0 && (((uintptr_t)status) & 7) == 0,
              "probs / label / keys must be 4-byte aligned, status 8-byte aligned");
  const int tv = C > 32 ? 128 : 256;   // at most 33 KB of LDS
  const long ntiles = (voxels + tv - 1) / tv;
  long blocks = 8L * ctx->num_cu;
  if (blocks > ntiles) blocks = ntiles;
  msk_launch_scope ls(ctx, "auc_pack");
  hipLaunchKernelGGL(auc_pack_k, dim3((unsigned)blocks), dim3(kThreads), (size_t)tv * (C | 1) * sizeof(uint32_t), ctx->stream,
                     (const float*)probs.p, probs.ld, voxels, C, label, keys, capacity, offset, tv, status);
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

int msk_auc_workspace(long count, int classes, size_t* bytes) {
  if (bytes == nullptr || count < 1 || count > 0x7fffffffL || classes < 1 || classes > 64)
    return msk_fail(nullptr, __FILE__, __LINE__, "msk_auc_workspace", "count must be in [1, 2^31), classes in [1,64], bytes not null");
  *bytes = auc_layout(count, classes).total;
  return 0;
}

int msk_auc_counts(msk_ctx* ctx, uint32_t* keys, long capacity, long count, int classes, void* workspace, size_t workspace_bytes,
                   unsigned long long* out) {
  MSK_REQUIRE(ctx, classes >= 1 && classes <= 64, "classes must be in [1,64]");
  MSK_REQUIRE(ctx, count >= 1 && count <= 0x7fffffffL, "count must be in [1, 2^31) keys per class");
  MSK_REQUIRE(ctx, capacity >= count, "count exceeds capacity");
  MSK_REQUIRE(ctx, keys != nullptr && workspace != nullptr && out != nullptr, "null keys / workspace / out");
  MSK_REQUIRE(ctx, (((uintptr_t)keys) & 3) == 0 && (((uintptr_t)workspace) & 15) == 0 && (((uintptr_t)out) & 7) == 0,
              "keys must be 4-byte aligned, workspace 16-byte, out 8-byte");
  const AucLayout L = auc_layout(count, classes);
  MSK_REQUIRE(ctx, workspace_bytes >= L.total, "workspace smaller than msk_auc_workspace(count, classes)");
  char* ws = (char*)workspace;
  uint32_t* scratch = (uint32_t*)(ws + L.scratch);
  uint32_t* hist = (uint32_t*)(ws + L.hist);
  uint32_t* part = (uint32_t*)(ws + L.part);
  uint32_t* blk = (uint32_t*)(ws + L.blk);
  const int n = (int)count, nb = L.nb, npart = L.npart;
  const dim3 chunks((unsigned)nb, (unsigned)classes);
  for (int pass = 0; pass < 4; ++pass) {
    const uint32_t* in = pass & 1 ? scratch : keys;
    uint32_t* dst = pass & 1 ? keys : scratch;
    const size_t is = pass & 1 ? L.stride : (size_t)capacity, os = pass & 1 ? (size_t)capacity : L.stride;
    const int shift = 8 * pass;
    const uint32_t mask = pass == 3 ? 127u : 255u;   // bit 31 is carried, never sorted on
    {
      msk_launch_scope ls(ctx, "auc_hist");
      hipLaunchKernelGGL(auc_hist_k, chunks, dim3(kThreads), 0, ctx->stream, in, is, n, nb, shift, mask, hist);
      MSK_LAUNCH_CHECK(ctx);
    }
    {
      msk_launch_scope ls(ctx, "auc_scan");
      hipLaunchKernelGGL(auc_scan_tiles_k, dim3((unsigned)npart, (unsigned)classes), dim3(kScanThreads), 0, ctx->stream, hist,
                         256 * nb, npart, part);
      MSK_LAUNCH_CHECK(ctx);
      hipLaunchKernelGGL(auc_scan_parts_k, dim3(1, (unsigned)classes), dim3(kScanThreads), 0, ctx->stream, part, npart);
      MSK_LAUNCH_CHECK(ctx);
    }
    {
      msk_launch_scope ls(ctx, "auc_scatter");
      hipLaunchKernelGGL(auc_scatter_k, chunks, dim3(kThreads), 0, ctx->stream, in, is, dst, os, n, nb, npart, shift, mask,
                         (const uint32_t*)hist, (const uint32_t*)part);
      MSK_LAUNCH_CHECK(ctx);
    }
  }
  msk_launch_scope ls(ctx, "auc_count");
  hipLaunchKernelGGL(auc_blocks_k, chunks, dim3(kThreads), 0, ctx->stream, (const uint32_t*)keys, (size_t)capacity, n, nb, blk);
  MSK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(auc_carry_k, dim3(1, (unsigned)classes), dim3(kScanThreads), 0, ctx->stream, blk, nb, n, out);
  MSK_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(auc_sum_k, chunks, dim3(kThreads), 0, ctx->stream, (const uint32_t*)keys, (size_t)capacity, n, nb,
                     (const uint32_t*)blk, out);
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
