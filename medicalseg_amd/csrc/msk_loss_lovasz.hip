// Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018; PaddleSeg's LovaszSoftmaxLoss) on an exact key-index radix SORT: per
// (group, class) plane the softmax errors e_v = |[y_v == c] - p_vc| in descending order, the gradient of the Jaccard index along
// that order, and the fixed-order float64 sum of their products, all on the device.  tests/lovasz_reference.py is the statement;
// include/msegk.h gives the record, the workspace layout and the formulas.  A group is the batch, or one sample with per_image.
//
//   pack      lv_pack_k: a thread owns a voxel (the thread-per-voxel scaffold of msk_device.h, the three record forms of
//             msk_loss_region.hip), takes the softmax and writes one 32-bit key per class plane.  An error is a float in [0, 1], so
//             its bit pattern b <= 0x3f800000 is already in float order; the key is 0x3f800000 - b in bits 0-29 (ASCENDING key =
//             DESCENDING error: reading an ascending stable sort backwards would reverse the tie order) and [y == c] in bit 31,
//             which is carried and never sorted on.  A voxel that takes no part (label ignore_index or outside [0, C)) gets
//             0x3fffffff in every plane: above the key 0x3f800000 of a valid voxel whose error is exactly 0, so the two never
//             interleave and the valid voxels are the first n_valid positions.
//   sort      a stable LSD radix sort of (key, voxel index) pairs on bits 0-29: digits of 8, 8, 8 and 6 bits, ping-pong between
//             two pairs of planes.  A pass is histogram -> exclusive scan -> stable scatter over chunks of 4096 keys, as in
//             msk_auc.hip (whose kernels sort keys alone; this file keeps its own: sharing the core was tried and taken back).  The
//             first pass reads no index (it is the position), the others move 20 bytes per key.  All planes in one launch
//             (gridDim.y); every dependency between workgroups is a kernel boundary; integer atomics in LDS histograms only.
//   scan/sum  lv_blocks_k: foreground and valid keys per chunk.  lv_carry_k (one workgroup per plane): the exclusive prefix of
//             the foreground counts, G and n_valid into the record.  lv_sum_k: cf_i from ballots and that prefix, then
//             J_i = 1 - (G - cf_i) / (G + i + 1 - cf_i), g_i = J_i - J_{i-1} in float64 from exact integers (one division, every
//             subtraction rounded on its own: the file compiles without contraction), the chunk's sum of float64(e_(i)) * g_i in
//             the order of msk_red_chunk's statement (lane l of 256 adds positions l, l + 256, ..., then the tree), and the
//             delivery of float32(g_i * scale) to voxel index_i of the class's dL/de plane (0 to a voxel that takes no part).  The
//             classes that count, and with them the scale 1 / (groups * counted classes of the group), come from the G of the
//             group's planes: every workgroup recounts them from the record.
//   finish    lv_finish_k: msk_red_finish over a plane's chunk values; lv_loss_k: the means, out and the tail of the record.
//   backward  lv_bwd_k: one thread-per-voxel pass recomputes the softmax, reads the C floats of dL/de and writes or adds
//             dz_k = coef p_k (s_k ge_k - sum_c s_c ge_c p_c), s_c = -1 at the label and +1 elsewhere, in a form that does not
//             cancel where the softmax is nearly one-hot (with classes='all' an absent class puts all of its weight on the
//             voxel most sure of it).  A voxel that takes no part gets zeros; when the pass adds, the lane's-own form skips
//             it and the LDS-tile forms add +0.0 to it (the value stays, a stored -0.0 becomes +0.0).
// Nothing is downloaded, nothing synchronises, no float atomics: two calls give the same bits.  22 launches forward, 1 backward.
#include <cmath>

#include "msk_common.h"

#pragma clang fp contract(off)   // for the whole file: J, g and the products e * g are rounded operation by operation

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kTpvThreads, "the tpv_* helpers of msk_device.h assume this workgroup");
constexpr int kIpt = 16;                    // keys per thread
constexpr int kChunk = kThreads * kIpt;     // keys per workgroup
static_assert(kChunk == kMskRedChunk && kThreads == kMskRedLanes, "a chunk of the sort is a chunk of the fixed-order sum");
constexpr int kScanThreads = 1024;
constexpr int kScanTile = 4 * kScanThreads; // histogram entries per workgroup of the first scan kernel
constexpr int kPasses = 4;                  // digits of 8, 8, 8 and 6 bits
constexpr uint32_t kOne = 0x3f800000u;      // the bits of 1.0f
constexpr uint32_t kKeyMask = 0x3fffffffu;  // the sorted bits
constexpr uint32_t kInvalid = 0x3fffffffu;  // a voxel that takes no part
constexpr uint32_t kFg = 0x80000000u;
constexpr int kStatsPerPlane = 4;           // {n_valid, G, L, scale}

enum { kClassesPresent = 0, kClassesAll = 1, kClassesList = 2 };

// p = softmax over zz[0..C) in place: the row maximum, expf, the sum in ascending class order, one division per class (p <= 1)
template <int CM>
__device__ __forceinline__ void lv_softmax(float (&zz)[CM], int C) {
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
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) zz[c] = zz[c] / se;
}

// ---- pack ------------------------------------------------------------------------------------------------------------------------
// keys: plane (group * C + c) at keys + plane * stride, a voxel at its raster position inside its group
template <int CM, int ST>
__global__ void __launch_bounds__(kThreads)
lv_pack_k(const float* __restrict__ z, int ld, const int32_t* __restrict__ labels, int ignore_index, long V, long Vg, int C,
          uint32_t* __restrict__ keys, size_t stride) {
  __shared__ float4 tile[tpv_tile_quads(CM, ST)];
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
    if (!mine) continue;                                 // (the barriers of the next round's fill are reached by everyone)
    const long grp = v / Vg;
    uint32_t* dst = keys + (size_t)grp * C * stride + (size_t)(v - grp * Vg);
    if (valid) {
      float zz[CM];
      tpv_take<CM, ST>(zz, tile, z + v * ld, C);
      lv_softmax<CM>(zz, C);
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) {
          const float e = fminf(fabsf((c == y ? 1.f : 0.f) - zz[c]), 1.f);
          dst[(size_t)c * stride] = (kOne - __float_as_uint(e)) | (c == y ? kFg : 0u);
        }
    } else {
      for (int c = 0; c < C; ++c) dst[(size_t)c * stride] = kInvalid;
    }
  }
}

// ---- sort: one digit pass --------------------------------------------------------------------------------------------------------
// hist[plane][digit * nb + chunk], nb = chunks of a plane
__global__ void __launch_bounds__(kThreads)
lv_hist_k(const uint32_t* __restrict__ in, size_t stride, int count, int nb, int shift, uint32_t mask, int agg,
          uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const uint32_t* kc = in + (size_t)blockIdx.y * stride;
  h[threadIdx.x] = 0;
  const long beg = (long)blockIdx.x * kChunk;
  uint32_t key[kIpt];
#pragma unroll
  for (int r = 0; r < kIpt; ++r) {
    const long i = beg + r * kThreads + (long)threadIdx.x;
    key[r] = i < count ? kc[i] : 0;
  }
  __syncthreads();
  // agg (the two upper digits): the exponent bits of neighbouring errors agree and every voxel that takes no part carries one
  // key, so most lanes of a wavefront hold one digit: msk_count_slot adds them with one LDS atomic.  The two lower digits are
  // mantissa bits, spread over the bins: one atomic per lane.  The counts are the same either way.
#pragma unroll
  for (int r = 0; r < kIpt; ++r) {
    const bool have = beg + r * kThreads + (long)threadIdx.x < count;
    const int dg = (int)((key[r] >> shift) & mask);
    if (agg) msk_count_slot(have ? dg : -1, h, threadIdx.x & 63);
    else if (have) atomicAdd(&h[dg], 1u);
  }
  __syncthreads();
  hist[(size_t)blockIdx.y * 256 * nb + (size_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan inside every tile of kScanTile entries; the tile's sum goes to part[plane][tile]
__global__ void __launch_bounds__(kScanThreads)
lv_scan_tiles_k(uint32_t* __restrict__ hist, int total, int npart, uint32_t* __restrict__ part) {
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

// exclusive scan of the npart tile sums of a plane, one workgroup per plane
__global__ void __launch_bounds__(kScanThreads)
lv_scan_parts_k(uint32_t* __restrict__ part, int npart) {
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

// stable scatter of (key, index): rounds of 256 keys in order; a lane's place among the equal digits of its wavefront comes from
// eight ballots, the wavefronts before it from LDS counts, the rounds before it from a running offset per digit.  FIRST: the
// index of a key is its position (the pass reads no index plane).
template <bool FIRST>
__global__ void __launch_bounds__(kThreads)
lv_scatter_k(const uint32_t* __restrict__ in, const uint32_t* __restrict__ in_idx, uint32_t* __restrict__ out,
             uint32_t* __restrict__ out_idx, size_t stride, int count, int nb, int npart, int shift, uint32_t mask,
             const uint32_t* __restrict__ hist, const uint32_t* __restrict__ part) {
  constexpr int NW = kThreads / 64;
  __shared__ uint32_t run[256];
  __shared__ uint32_t wcnt[NW][256];
  const uint32_t* kc = in + (size_t)blockIdx.y * stride;
  const uint32_t* ic = in_idx + (size_t)blockIdx.y * stride;
  uint32_t* oc = out + (size_t)blockIdx.y * stride;
  uint32_t* oi = out_idx + (size_t)blockIdx.y * stride;
  const uint32_t* hc = hist + (size_t)blockIdx.y * 256 * nb;
  const uint32_t* pc = part + (size_t)blockIdx.y * npart;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {
    const int e = tid * nb + (int)blockIdx.x;
    run[tid] = hc[e] + pc[e / kScanTile];
  }
  const unsigned long long lt = (1ull << lane) - 1ull;
  const long beg = (long)blockIdx.x * kChunk;
  uint32_t key[kIpt], idx[kIpt];
#pragma unroll
  for (int r = 0; r < kIpt; ++r) {
    const long i = beg + r * kThreads + tid;
    key[r] = i < count ? kc[i] : 0;
    idx[r] = FIRST ? (uint32_t)i : (i < count ? ic[i] : 0);
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
      if (pos < (uint32_t)count) {             // always true for a correct histogram: a guard, not a case
        oc[pos] = key[r];
        oi[pos] = idx[r];
      }
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

// ---- scan and sum ------------------------------------------------------------------------------------------------------------------
// per chunk of the sorted keys: blk[plane][chunk] = foreground keys, blk[plane][nb + chunk] = valid keys
__global__ void __launch_bounds__(kThreads)
lv_blocks_k(const uint32_t* __restrict__ keys, size_t stride, int count, int nb, uint32_t* __restrict__ blk) {
  __shared__ uint32_t wtot[kThreads / 64];
  const uint32_t* kc = keys + (size_t)blockIdx.y * stride;
  const long beg = (long)blockIdx.x * kChunk;
  uint32_t nfg = 0, nval = 0;
#pragma unroll
  for (int r = 0; r < kIpt; ++r) {
    const long i = beg + r * kThreads + (long)threadIdx.x;
    if (i < count) {
      const uint32_t k = kc[i];
      nfg += k >> 31;
      nval += (k & kKeyMask) != kInvalid ? 1u : 0u;
    }
  }
  uint32_t allfg, allval;
  msk_block_excl_scan<false>(nfg, 0u, msk_op_add(), wtot, &allfg);
  msk_block_excl_scan<false>(nval, 0u, msk_op_add(), wtot, &allval);
  if (threadIdx.x == 0) {
    uint32_t* b = blk + (size_t)blockIdx.y * 2 * nb;
    b[blockIdx.x] = allfg;
    b[nb + blockIdx.x] = allval;
  }
}

// One workgroup per plane over the nb chunk counts, a thread owning a contiguous segment of them.  In place: blk[0] -> foreground
// keys in front of the chunk.  stats[plane] = {n_valid, G, ., .}
__global__ void __launch_bounds__(kScanThreads)
lv_carry_k(uint32_t* __restrict__ blk, int nb, double* __restrict__ stats) {
  __shared__ uint32_t wtot[kScanThreads / 64];
  uint32_t* fgv = blk + (size_t)blockIdx.y * 2 * nb;
  const uint32_t* valv = fgv + nb;
  const int seg = (nb + kScanThreads - 1) / kScanThreads;
  const int b0 = min(nb, (int)threadIdx.x * seg), b1 = min(nb, b0 + seg);
  uint32_t s = 0, sv = 0;
  for (int b = b0; b < b1; ++b) {
    s += fgv[b];
    sv += valv[b];
  }
  uint32_t G, nvalid;
  uint32_t run = msk_block_excl_scan<false>(s, 0u, msk_op_add(), wtot, &G);
  msk_block_excl_scan<false>(sv, 0u, msk_op_add(), wtot, &nvalid);
  for (int b = b0; b < b1; ++b) {
    const uint32_t n = fgv[b];
    fgv[b] = run;
    run += n;
  }
  if (threadIdx.x == 0) {
    double* st = stats + (size_t)blockIdx.y * kStatsPerPlane;
    st[0] = (double)nvalid;
    st[1] = (double)G;
  }
}

// does class c of a group count, given the G of its plane?
__device__ __forceinline__ bool lv_counted(int mode, unsigned long long mask, int c, double G) {
  if (mode == kClassesAll) return true;
  if (mode == kClassesList && !((mask >> c) & 1ull)) return false;
  return G > 0.0;
}

// J at the 1-based position i1 with cf foreground keys at or in front of it: exact integers, one division, one subtraction
__device__ __forceinline__ double lv_jaccard(long G, long i1, long cf) {
  return 1.0 - (double)(G - cf) / (double)(G + i1 - cf);
}

// A workgroup per chunk and plane.  Thread t is lane t of the fixed-order sum: it takes the positions beg + 256 r + t.
__global__ void __launch_bounds__(kThreads)
lv_sum_k(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ idx, size_t stride, int count, int nb, int C, int groups,
         int mode, unsigned long long mask, const uint32_t* __restrict__ blk, double* __restrict__ stats,
         float* __restrict__ ge, double* __restrict__ partial) {
  __shared__ uint32_t s_cnt[kIpt * (kThreads / 64)];
  __shared__ int s_ncounted;
  __shared__ double s_t[kThreads];
  const int plane = blockIdx.y, grp = plane / C, cls = plane - grp * C;
  const uint32_t* kc = keys + (size_t)plane * stride;
  const uint32_t* ic = idx + (size_t)plane * stride;
  float* gc = ge + (size_t)plane * stride;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long beg = (long)blockIdx.x * kChunk;
  uint32_t key[kIpt], vox[kIpt];
#pragma unroll
  for (int r = 0; r < kIpt; ++r) {
    const long i = beg + r * kThreads + tid;
    key[r] = i < count ? kc[i] : kInvalid;
    vox[r] = i < count ? ic[i] : 0u;
  }
  const double* st = stats + (size_t)plane * kStatsPerPlane;
  const long nvalid = (long)st[0], G = (long)st[1];
  if (tid < 64) {                                         // the classes of this group that count
    const bool cnt = tid < C && lv_counted(mode, mask, tid, stats[((size_t)grp * C + tid) * kStatsPerPlane + 1]);
    const unsigned long long b = __ballot(cnt);
    if (tid == 0) s_ncounted = __popcll(b);
  }
  const unsigned long long le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  int pre[kIpt];                                          // foreground keys of the wavefront's round at or in front of this lane
#pragma unroll
  for (int r = 0; r < kIpt; ++r) {
    const bool fg = beg + r * kThreads + tid < nvalid && (key[r] >> 31);
    const unsigned long long b = __ballot(fg);
    pre[r] = __popcll(b & le);
    if (lane == 0) s_cnt[r * (kThreads / 64) + wave] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (tid < 64) {                                         // 16 rounds x 4 wavefronts, in position order
    const uint32_t v = s_cnt[tid];
    const uint32_t inc = msk_wave_incl_scan<false>(v, msk_op_add());
    s_cnt[tid] = inc - v;
  }
  __syncthreads();
  const double scale = lv_counted(mode, mask, cls, (double)G) ? 1.0 / ((double)groups * (double)s_ncounted) : 0.0;
  if (blockIdx.x == 0 && tid == 0) stats[(size_t)plane * kStatsPerPlane + 3] = scale;
  const long cbase = (long)blk[(size_t)plane * 2 * nb + blockIdx.x];
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < kIpt; ++r) {
    const long i = beg + r * kThreads + tid;
    double term = 0.0;                                    // a position past n_valid adds the statement's + 0.0
    if (i < nvalid) {
      const long cf = cbase + (long)s_cnt[r * (kThreads / 64) + wave] + pre[r];
      const long cfp = cf - (long)(key[r] >> 31);
      const double J = lv_jaccard(G, i + 1, cf);
      const double Jp = i == 0 ? 0.0 : lv_jaccard(G, i, cfp);
      const double g = J - Jp;
      const double e = (double)__uint_as_float(kOne - (key[r] & kKeyMask));
      term = e * g;
      if (vox[r] < (uint32_t)count) gc[vox[r]] = (float)(g * scale);   // always true for a permutation: a guard, not a case
    } else if (i < count && vox[r] < (uint32_t)count) {
      gc[vox[r]] = 0.f;
    }
    acc = acc + term;
  }
  s_t[tid] = acc;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) s_t[tid] = s_t[tid] + s_t[tid + o];
    __syncthreads();
  }
  if (tid == 0) partial[(size_t)plane * nb + blockIdx.x] = s_t[0];
}

// one workgroup of 256 per plane: L = the chunk values in the order of msk_red_finish
__global__ void __launch_bounds__(kMskRedLanes)
lv_finish_k(int nb, const double* __restrict__ partial, double* __restrict__ stats) {
  const msk_red_vals red = msk_red_finish<false>(nb, nullptr, partial + (size_t)blockIdx.x * nb, nullptr, nullptr);
  if (threadIdx.x == 0) stats[(size_t)blockIdx.x * kStatsPerPlane + 2] = red.sumsq;
}

// one workgroup of 64.  loss = (sum over groups of (sum over its counted classes, ascending, of L) / their number) / groups;
// out = {loss, counted (group, class) pairs, per class the mean L over the groups that count it}; stats tail = {loss, pairs}
__global__ void __launch_bounds__(64)
lv_loss_k(int groups, int C, double* __restrict__ stats, float* __restrict__ out) {
  const int t = threadIdx.x;
  if (t < C) {
    double s = 0.0;
    int k = 0;
    for (int g = 0; g < groups; ++g) {
      const double* st = stats + ((size_t)g * C + t) * kStatsPerPlane;
      if (st[3] != 0.0) {
        s = s + st[2];
        ++k;
      }
    }
    out[2 + t] = k ? (float)(s / (double)k) : 0.f;
  }
  if (t == 0) {
    double tot = 0.0;
    long pairs = 0;
    for (int g = 0; g < groups; ++g) {
      double s = 0.0;
      int k = 0;
      for (int c = 0; c < C; ++c) {
        const double* st = stats + ((size_t)g * C + c) * kStatsPerPlane;
        if (st[3] != 0.0) {
          s = s + st[2];
          ++k;
        }
      }
      if (k) tot = tot + s / (double)k;
      pairs += k;
    }
    const double loss = tot / (double)groups;
    double* tail = stats + (size_t)groups * C * kStatsPerPlane;
    tail[0] = loss;
    tail[1] = (double)pairs;
    out[0] = (float)loss;
    out[1] = (float)pairs;
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// dz (+)= coef p_k (s_k ge_k - sum_c s_c ge_c p_c); a voxel that takes no part gets zeros (nothing when the pass adds)
template <int CM, int ST>
__global__ void __launch_bounds__(kThreads)
lv_bwd_k(const float* __restrict__ z, int ld, const int32_t* __restrict__ labels, int ignore_index, const float* __restrict__ ge,
         size_t stride, long Vg, float coef, int accumulate, float* __restrict__ dz, int lddz, long V, int C) {
  __shared__ float4 tile[tpv_tile_quads(CM, ST)];
  const long ntile = (V + kThreads - 1) / kThreads;
  for (long it = blockIdx.x; it < ntile; it += gridDim.x) {
    const long v0 = it * kThreads;
    const long left = V - v0;
    const int nv = (int)(left < kThreads ? left : kThreads);
    const bool mine = (int)threadIdx.x < nv;
    const long v = v0 + (mine ? threadIdx.x : 0);
    const int y = mine ? labels[v] : ignore_index;
    const bool valid = mine && y != ignore_index && (unsigned)y < (unsigned)C;
    float gg[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) gg[c] = 0.f;
    if (valid) {                                          // the C floats of dL/de, asked for ahead of the tile
      const long grp = v / Vg;
      const float* gp = ge + (size_t)grp * C * stride + (size_t)(v - grp * Vg);
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) gg[c] = gp[(size_t)c * stride];
    }
    tpv_fill<CM, ST>(tile, z + v0 * C, nv, C);
    if (valid) {
      float zz[CM];
      tpv_take<CM, ST>(zz, tile, z + v * ld, C);
      lv_softmax<CM>(zz, C);
      // a_c = s_c ge_c.  a_k - sum_c a_c p_c cancels where the softmax is nearly one-hot at k (1 - p_k in float32); with m the
      // class of the largest probability it is (a_k - a_m) + sum_c p_c (a_m - a_c), whose term c = m is exactly 0
      float pm = -1.f, am = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) {
          gg[c] = c == y ? -gg[c] : gg[c];
          if (zz[c] > pm) {
            pm = zz[c];
            am = gg[c];
          }
        }
      float dm = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) dm += zz[c] * (am - gg[c]);
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) gg[c] = coef * (zz[c] * ((gg[c] - am) + dm));
    }
    if (ST) {
      tpv_put<CM, ST>(gg, tile, dz + v0 * C, C, nv, mine, accumulate != 0);
    } else if (mine && (valid || !accumulate)) {
      float* dp = dz + v * lddz;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) dp[c] = accumulate ? dp[c] + gg[c] : gg[c];
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
// workspace: sorted keys | their voxel indices | the dL/de planes (the second key buffer of the sort) | the second index buffer |
// histograms | tile sums | chunk counts | chunk values; every part on a 256-byte boundary, planes of `stride` words
struct LvLayout {
  size_t stride;    // words per plane
  int nb, npart;
  size_t keys, idx, ge, idx2, hist, part, blk, partial, total;   // byte offsets
};

inline size_t lv_up256(size_t b) { return (b + 255) & ~(size_t)255; }

inline LvLayout lv_layout(long count, long planes) {
  LvLayout L;
  L.stride = ((size_t)count + 63) & ~(size_t)63;
  L.nb = (int)((count + kChunk - 1) / kChunk);
  L.npart = (int)(((long)256 * L.nb + kScanTile - 1) / kScanTile);
  const size_t plane_bytes = lv_up256((size_t)planes * L.stride * 4);
  L.keys = 0;
  L.idx = plane_bytes;
  L.ge = 2 * plane_bytes;
  L.idx2 = 3 * plane_bytes;
  L.hist = 4 * plane_bytes;
  L.part = lv_up256(L.hist + (size_t)planes * 256 * L.nb * 4);
  L.blk = lv_up256(L.part + (size_t)planes * L.npart * 4);
  L.partial = lv_up256(L.blk + (size_t)planes * 2 * L.nb * 4);
  L.total = lv_up256(L.partial + (size_t)planes * L.nb * 8);
  return L;
}

// the record form of a call: 2 = flat LDS tile (dense, C <= 4), 1 = quad tile (dense, C % 4 == 0, C <= 32), 0 = a lane's own
inline int lv_form(int C, bool dense) { return !dense ? 0 : (C <= 4 ? 2 : ((C % 4 == 0 && C <= 32) ? 1 : 0)); }

int lv_check(msk_ctx* ctx, const msk_tensor& logits, const int32_t* labels, int per_image, const void* workspace,
             size_t workspace_bytes, const double* stats, LvLayout* layout) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, logits.p != nullptr && labels != nullptr && workspace != nullptr && stats != nullptr,
              "null logits / labels / workspace / stats");
  MSK_REQUIRE(ctx, logits.c >= 2 && logits.c <= 64, "num_classes must be in [2,64]");
  MSK_REQUIRE(ctx, logits.ld >= logits.c, "logits.ld must be >= logits.c");
  MSK_REQUIRE(ctx, logits.n >= 1 && logits.d >= 1 && logits.h >= 1 && logits.w >= 1, "empty logits");
  const long groups = per_image ? logits.n : 1;
  const long Vg = msk_voxels(logits) / groups;
  MSK_REQUIRE(ctx, Vg <= 0x7fffffffL, "voxels per group must be below 2^31");
  MSK_REQUIRE(ctx, groups * logits.c <= 65535, "groups x classes must be at most 65535");
  MSK_REQUIRE(ctx, ((((uintptr_t)logits.p) | ((uintptr_t)labels)) & 3) == 0, "logits / labels must be 4-byte aligned");
  MSK_REQUIRE(ctx, (((uintptr_t)workspace) & 15) == 0 && (((uintptr_t)stats) & 7) == 0,
              "workspace must be 16-byte, stats 8-byte aligned");
  *layout = lv_layout(Vg, groups * logits.c);
  MSK_REQUIRE(ctx, workspace_bytes >= layout->total, "workspace smaller than msk_lovasz_workspace(voxels, classes, groups)");
  const long V = msk_voxels(logits);
  const size_t wb = layout->total, sb = ((size_t)groups * logits.c * kStatsPerPlane + 2) * 8;
  MSK_REQUIRE(ctx, msk_bytes_disjoint(workspace, wb, logits.p, ((size_t)(V - 1) * logits.ld + logits.c) * 4) &&
                       msk_bytes_disjoint(workspace, wb, labels, (size_t)V * 4) && msk_bytes_disjoint(workspace, wb, stats, sb),
              "workspace overlaps an operand");
  return 0;
}

}  // namespace

// CM: register arrays sized to the class count in steps of a quad, as the region kernels do; 33..64 classes take the lane's-own
// form only
#define LV_DISPATCH(LAUNCH)                                     \
  do {                                                          \
    if (C <= 4) { if (st == 2) LAUNCH(4, 2); else LAUNCH(4, 0); } \
    else if (C <= 32) MSK_TPV_LADDER(C, st == 1, LAUNCH);       \
    else LAUNCH(64, 0);                                         \
  } while (0)

extern "C" {

int msk_lovasz_workspace(long voxels, int classes, int groups, size_t* bytes) {
  MSK_REQUIRE(nullptr, bytes != nullptr, "bytes must not be null");
  MSK_REQUIRE(nullptr, voxels >= 1 && voxels <= 0x7fffffffL, "voxels per group must be in [1, 2^31)");
  MSK_REQUIRE(nullptr, classes >= 2 && classes <= 64, "classes must be in [2,64]");
  MSK_REQUIRE(nullptr, groups >= 1 && (long)groups * classes <= 65535, "groups x classes must be in [1, 65535]");
  *bytes = lv_layout(voxels, (long)groups * classes).total;
  return 0;
}

int msk_lovasz_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, int class_mode,
                   unsigned long long class_mask, int per_image, void* workspace, size_t workspace_bytes, float* out,
                   double* stats) {
  LvLayout L;
  if (lv_check(ctx, logits, labels, per_image, workspace, workspace_bytes, stats, &L)) return -1;
  MSK_REQUIRE(ctx, out != nullptr && (((uintptr_t)out) & 3) == 0, "out must be a 4-byte aligned pointer");
  MSK_REQUIRE(ctx, class_mode >= kClassesPresent && class_mode <= kClassesList, "class_mode must be 0 (present), 1 (all) or 2 (list)");
  const int C = logits.c;
  MSK_REQUIRE(ctx, class_mode != kClassesList || (C == 64 ? class_mask != 0 : (class_mask != 0 && (class_mask >> C) == 0)),
              "class_mask must name at least one class, and none outside [0, C)");
  MSK_REQUIRE(ctx, msk_bytes_disjoint(workspace, L.total, out, (size_t)(2 + C) * 4), "workspace overlaps an operand");
  const long V = msk_voxels(logits);
  const int groups = per_image ? logits.n : 1;
  const long Vg = V / groups;
  const int planes = groups * C, n = (int)Vg, nb = L.nb, npart = L.npart;
  char* ws = (char*)workspace;
  uint32_t* keys = (uint32_t*)(ws + L.keys);
  uint32_t* idx = (uint32_t*)(ws + L.idx);
  uint32_t* keys2 = (uint32_t*)(ws + L.ge);
  uint32_t* idx2 = (uint32_t*)(ws + L.idx2);
  uint32_t* hist = (uint32_t*)(ws + L.hist);
  uint32_t* part = (uint32_t*)(ws + L.part);
  uint32_t* blk = (uint32_t*)(ws + L.blk);
  double* partial = (double*)(ws + L.partial);
  const int st = lv_form(C, msk_quad_dense(logits));
  {
    msk_launch_scope ls(ctx, "lovasz_pack");
    const int nblk = msk_ew_blocks(V, ctx->num_cu, 8);
#define LV_PACK(CM_, ST_)                                                                                                      \
  hipLaunchKernelGGL((lv_pack_k<CM_, ST_>), dim3(nblk), dim3(kThreads), 0, ctx->stream, (const float*)logits.p, logits.ld, labels, \
                     ignore_index, V, Vg, C, keys, L.stride)
    LV_DISPATCH(LV_PACK);
#undef LV_PACK
    MSK_LAUNCH_CHECK(ctx);
  }
  const dim3 chunks((unsigned)nb, (unsigned)planes);
  for (int pass = 0; pass < kPasses; ++pass) {          // keys -> keys2 -> keys -> keys2 -> keys
    const uint32_t* in = pass & 1 ? keys2 : keys;
    const uint32_t* in_idx = pass & 1 ? idx2 : idx;
    uint32_t* dst = pass & 1 ? keys : keys2;
    uint32_t* dst_idx = pass & 1 ? idx : idx2;
    const int shift = 8 * pass;
    const uint32_t mask = pass == kPasses - 1 ? 63u : 255u;   // bits 30 and 31 are carried, never sorted on
    {
      msk_launch_scope ls(ctx, "lovasz_hist");
      hipLaunchKernelGGL(lv_hist_k, chunks, dim3(kThreads), 0, ctx->stream, in, L.stride, n, nb, shift, mask, pass >= 2 ? 1 : 0, hist);
      MSK_LAUNCH_CHECK(ctx);
    }
    {
      msk_launch_scope ls(ctx, "lovasz_scan");
      hipLaunchKernelGGL(lv_scan_tiles_k, dim3((unsigned)npart, (unsigned)planes), dim3(kScanThreads), 0, ctx->stream, hist,
                         256 * nb, npart, part);
      MSK_LAUNCH_CHECK(ctx);
      hipLaunchKernelGGL(lv_scan_parts_k, dim3(1, (unsigned)planes), dim3(kScanThreads), 0, ctx->stream, part, npart);
      MSK_LAUNCH_CHECK(ctx);
    }
    {
      msk_launch_scope ls(ctx, "lovasz_scatter");
      if (pass == 0)
        hipLaunchKernelGGL((lv_scatter_k<true>), chunks, dim3(kThreads), 0, ctx->stream, in, in_idx, dst, dst_idx, L.stride, n, nb,
                           npart, shift, mask, (const uint32_t*)hist, (const uint32_t*)part);
      else
        hipLaunchKernelGGL((lv_scatter_k<false>), chunks, dim3(kThreads), 0, ctx->stream, in, in_idx, dst, dst_idx, L.stride, n, nb,
                           npart, shift, mask, (const uint32_t*)hist, (const uint32_t*)part);
      MSK_LAUNCH_CHECK(ctx);
    }
  }
  {
    msk_launch_scope ls(ctx, "lovasz_scan_fg");
    hipLaunchKernelGGL(lv_blocks_k, chunks, dim3(kThreads), 0, ctx->stream, (const uint32_t*)keys, L.stride, n, nb, blk);
    MSK_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(lv_carry_k, dim3(1, (unsigned)planes), dim3(kScanThreads), 0, ctx->stream, blk, nb, stats);
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "lovasz_sum");
    hipLaunchKernelGGL(lv_sum_k, chunks, dim3(kThreads), 0, ctx->stream, (const uint32_t*)keys, (const uint32_t*)idx, L.stride, n,
                       nb, C, groups, class_mode, class_mask, (const uint32_t*)blk, stats, (float*)keys2, partial);
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "lovasz_finish");
    hipLaunchKernelGGL(lv_finish_k, dim3((unsigned)planes), dim3(kMskRedLanes), 0, ctx->stream, nb, (const double*)partial, stats);
    MSK_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(lv_loss_k, dim3(1), dim3(64), 0, ctx->stream, groups, C, stats, out);
    MSK_LAUNCH_CHECK(ctx);
  }
  return 0;
}

int msk_lovasz_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, int per_image, const void* workspace,
                   size_t workspace_bytes, const double* stats, float coef, int accumulate, msk_tensor dz) {
  LvLayout L;
  if (lv_check(ctx, logits, labels, per_image, workspace, workspace_bytes, stats, &L)) return -1;
  const int C = logits.c;
  const long V = msk_voxels(logits);
  MSK_REQUIRE(ctx, dz.p != nullptr && (((uintptr_t)dz.p) & 3) == 0, "dz must be a 4-byte aligned pointer");
  MSK_REQUIRE(ctx, msk_same_shape(logits, dz) && dz.ld >= C, "dz shape mismatch");
  MSK_REQUIRE(ctx, msk_bytes_disjoint(workspace, L.total, dz.p, ((size_t)(V - 1) * dz.ld + C) * 4), "workspace overlaps an operand");
  const int groups = per_image ? logits.n : 1;
  const long Vg = V / groups;
  const float* ge = (const float*)((const char*)workspace + L.ge);
  const int st = lv_form(C, msk_quad_dense(logits) && msk_quad_dense(dz));
  const int nblk = msk_ew_blocks(V, ctx->num_cu, 16);
  msk_launch_scope ls(ctx, "lovasz_bwd");
#define LV_BWD(CM_, ST_)                                                                                                     \
  hipLaunchKernelGGL((lv_bwd_k<CM_, ST_>), dim3(nblk), dim3(kThreads), 0, ctx->stream, (const float*)logits.p, logits.ld, labels, \
                     ignore_index, ge, L.stride, Vg, coef, accumulate, (float*)dz.p, dz.ld, V, C)
  LV_DISPATCH(LV_BWD);
#undef LV_BWD
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
