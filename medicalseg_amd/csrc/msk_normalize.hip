// Foreground statistics with two percentiles, percentile clipping + z-scoring, and the non-zero bounding box of a volume that
// lives on the device (nnU-Net's crop_to_nonzero / CTNormalization / ZScoreNormalization; preprocess.fg_stats_device,
// clip_zscore_device, nonzero_bbox_device).  tests/normalize_reference.py is the statement; include/msegk.h gives the records.
//
//   fg_stats   the radix select of msk_loss_topk.hip (keys, 2048-bin histograms and digit resolution: msk_sel_* of msk_device.h)
//              over the VALID voxels (all / x != 0 / mask > 0), with TWO ranks travelling through the same three passes: the
//              first digit is shared, passes 2 and 3 keep one LDS histogram per rank.  Nothing is packed: a pass re-evaluates
//              validity from x (and reads the mask, 4 more bytes per voxel, with MSK_MASK_LABEL only), so the workspace is the
//              histograms and 32 bytes per chunk.  K = n_valid - floor((n_valid - 1) q / 100) is evaluated on the device by
//              every workgroup from the n_valid the first pass counted (one global atomic per workgroup).
//   sum        fg_sum_k: msk_red_chunk's lanes and tree (a wavefront per chunk of 4096, four chunks per workgroup because
//              the prologue wants 256 threads) with an invalid voxel adding +0.0; the chunk's smallest and largest valid key
//              and, per rank, its smallest key ABOVE a = s[i] ride along.  The interpolation neighbour b = s[i + 1] needs no
//              second select: it is a when the ties at a reach rank i + 1, else the minimum above a.
//   finish     fg_finish_k: msk_red_finish over the chunk sums, integer min / max over the chunk keys, then the moments and the
//              two interpolations in float64, every operation rounded on its own (this file compiles with contraction off).
//   apply      clip_zscore_*_k: tiles of 1024 quads per workgroup in a grid-stride loop (msk_intensity_apply's map); the four
//              scalars come from the DEVICE record, read behind the thread's first loads, or from the host.  No float32 division.
//   bbox       nonzero_bbox_k: a workgroup takes tiles of 1024 quads of the flat volume (four loads per thread in flight), a thread
//              splits the flat index once per quad that holds a non-zero word (two 32-bit divisions) and steps the coordinates
//              inside it; a workgroup reduces six extremes and the count through shuffles and LDS and, only if it saw a non-zero
//              voxel, adds its count and sends those extremes that still move the record (at most seven integer atomics).  The
//              lower corner travels as extent - coordinate under atomicMax, so a memset initialises the record; a one-thread
//              finish turns it round.
// One memset and five launches (fg_stats), one launch (apply), one memset and two launches (bbox).  Integer atomics only; nothing
// is downloaded and nothing synchronises.
#include <cmath>

#include "msk_common.h"

#pragma clang fp contract(off)   // for the whole file: every multiply and add below is rounded on its own

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kMskSelThreads, "the msk_sel_* helpers of msk_device.h assume this workgroup");
constexpr int kBins = kMskSelBins;
constexpr int kRanks = 2;        // the two percentiles of a call

struct FgCtl {                   // zeroed by one memset per call
  uint32_t hist0[kBins];         // first digit of every valid key
  uint32_t hist[kRanks][2][kBins];   // [rank][pass - 1]
  uint32_t n_valid;
  uint32_t pad[63];
};
static_assert(sizeof(FgCtl) % 256 == 0, "the chunk values behind it stay aligned");

// workspace: FgCtl | sum[nc] | sumsq[nc] (doubles) | kmin[nc] | kmax[nc] | above[2][nc] (keys), each rounded up to 256 bytes
struct FgWs {
  FgCtl* ctl;
  double *psum, *psq;
  uint32_t *kmin, *kmax, *above[kRanks];
};
inline size_t fg_round256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t fg_ws_bytes(long n) {
  const size_t nc = (size_t)msk_chunks_of((size_t)n);
  return sizeof(FgCtl) + 2 * fg_round256(nc * 8) + 4 * fg_round256(nc * 4);
}
inline FgWs fg_ws(void* w, long n) {
  const size_t nc = (size_t)msk_chunks_of((size_t)n);
  FgWs s;
  char* p = (char*)w;
  s.ctl = (FgCtl*)p;                 p += sizeof(FgCtl);
  s.psum = (double*)p;               p += fg_round256(nc * 8);
  s.psq = (double*)p;                p += fg_round256(nc * 8);
  s.kmin = (uint32_t*)p;             p += fg_round256(nc * 4);
  s.kmax = (uint32_t*)p;             p += fg_round256(nc * 4);
  s.above[0] = (uint32_t*)p;         p += fg_round256(nc * 4);
  s.above[1] = (uint32_t*)p;
  return s;
}

__device__ __forceinline__ bool fg_valid(int mode, float x, int32_t m) {
  return mode == MSK_MASK_ALL ? true : (mode == MSK_MASK_NONZERO ? x != 0.f : m > 0);
}

// the rank of a percentile among nv valid values: h = (nv - 1) (q / 100), i = floor(h), g = h - i; K = nv - i is its rank from
// the top.  nv == 0: K = 0.
struct FgRank {
  uint32_t i, K;
  double g;
};
__device__ __forceinline__ FgRank fg_rank(uint32_t nv, double q) {
  FgRank r = {0u, 0u, 0.0};
  if (nv == 0) return r;
  const double h = (double)(nv - 1u) * (q / 100.0);
  const double fi = floor(h);
  r.g = h - fi;
  r.i = (uint32_t)fi;
  r.K = nv - r.i;
  return r;
}

struct FgSel {
  uint32_t nv;
  FgRank rank[kRanks];
  msk_sel sel[kRanks];
};
// the first NP digits of both ranks' keys from the global histograms; called by all 256 threads, everything asked for at once.
// nv == 0 returns before any barrier (uniform).
template <int NP>
__device__ __forceinline__ FgSel fg_resolve(const FgCtl* __restrict__ ctl, double q_lo, double q_hi, uint32_t* s_scan) {
  msk_sel_bins<NP> bins[kRanks];
#pragma unroll
  for (int t = 0; t < kRanks; ++t) {
    const uint32_t* hist[3] = {ctl->hist0, ctl->hist[t][0], ctl->hist[t][1]};
    bins[t] = msk_sel_load<NP>(hist);
  }
  FgSel s;
  s.nv = ctl->n_valid;
  s.rank[0] = fg_rank(s.nv, q_lo);
  s.rank[1] = fg_rank(s.nv, q_hi);
#pragma unroll
  for (int t = 0; t < kRanks; ++t) s.sel[t] = msk_sel_scan<NP>(bins[t], s.rank[t].K, s_scan);
  return s;
}

// digit P of the valid keys (P == 0: of all of them, and n_valid; else per rank of those that carry the rank's digits so far);
// grid-stride over quads (vec: x, and the mask when it is read, are 16-byte aligned) or single elements
template <int P>
__global__ void __launch_bounds__(kThreads)
fg_hist_k(const float* __restrict__ x, const int32_t* __restrict__ mask, long n, int mode, int vec, FgCtl* __restrict__ ctl,
          double q_lo, double q_hi) {
  constexpr int NH = P == 0 ? 1 : kRanks;
  __shared__ uint32_t s_hist[NH][kBins];
  __shared__ uint32_t s_scan[8];
  __shared__ uint32_t s_nvalid;
#pragma unroll
  for (int t = 0; t < NH; ++t) msk_sel_hist_clear(s_hist[t]);
  if (threadIdx.x == 0) s_nvalid = 0u;
  const long stride = (long)gridDim.x * kThreads;
  const long n4 = n >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const int4* m4 = reinterpret_cast<const int4*>(mask);
  const bool use_mask = mode == MSK_MASK_LABEL;
  // the first quad is asked for before the histograms of the passes before this one are
  long i = (long)blockIdx.x * kThreads + threadIdx.x;
  float4 cur = make_float4(0.f, 0.f, 0.f, 0.f);
  int4 curm = make_int4(1, 1, 1, 1);
  if (vec && i < n4) {
    cur = x4[i];
    if (use_mask) curm = m4[i];
  }
  uint32_t prefix[kRanks] = {0u, 0u};
  if (P > 0) {
    const FgSel s = fg_resolve<(P > 0 ? P : 1)>(ctl, q_lo, q_hi, s_scan);
    if (s.nv == 0) return;                               // uniform: the record is all zeros
    prefix[0] = s.sel[0].prefix;
    prefix[1] = s.sel[1].prefix;
  } else {
    __syncthreads();
  }
  constexpr int kShift = msk_sel_shift(P);
  constexpr uint32_t kMask = (1u << msk_sel_width(P)) - 1u;
  uint32_t nvalid = 0;
  auto count = [&](float f, int32_t m) {
    if (!fg_valid(mode, f, m)) return;
    const uint32_t key = msk_sel_key(f);
    const uint32_t digit = (key >> kShift) & kMask;
    if (P == 0) {
      ++nvalid;
      atomicAdd(&s_hist[0][digit], 1u);
    } else {
      const uint32_t head = key >> (kShift + msk_sel_width(P));
#pragma unroll
      for (int t = 0; t < NH; ++t)
        if (head == prefix[t]) atomicAdd(&s_hist[t][digit], 1u);
    }
  };
  if (vec) {
    while (i < n4) {
      const float4 v = cur;
      const int4 m = curm;
      i += stride;
      if (i < n4) {                                      // the next quad, ahead of the counting
        cur = x4[i];
        if (use_mask) curm = m4[i];
      }
      count(v.x, m.x); count(v.y, m.y); count(v.z, m.z); count(v.w, m.w);
    }
    if (blockIdx.x == 0) {                               // the last n % 4 elements
      const long e = 4 * n4 + threadIdx.x;
      if (threadIdx.x < 4 && e < n) count(x[e], use_mask ? mask[e] : 1);
    }
  } else {
    for (long e = (long)blockIdx.x * kThreads + threadIdx.x; e < n; e += stride) count(x[e], use_mask ? mask[e] : 1);
  }
  if (P == 0) {
    nvalid = msk_wave_sum_u32(nvalid);
    if ((threadIdx.x & 63) == 0 && nvalid) atomicAdd(&s_nvalid, nvalid);
  }
  __syncthreads();
  if (P == 0) {
    msk_sel_hist_merge(s_hist[0], ctl->hist0);
    if (threadIdx.x == 0 && s_nvalid) atomicAdd(&ctl->n_valid, s_nvalid);   // one single-word atomic per workgroup
  } else {
#pragma unroll
    for (int t = 0; t < NH; ++t) msk_sel_hist_merge(s_hist[t], ctl->hist[t][P - 1]);
  }
}

constexpr int kSumChunks = kThreads / 64;                // chunks per workgroup of fg_sum_k
constexpr uint32_t kNoKey = 0xffffffffu;                 // above every key of a finite value

__device__ __forceinline__ uint32_t fg_wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t fg_wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

__global__ void __launch_bounds__(kThreads)
fg_sum_k(const float* __restrict__ x, const int32_t* __restrict__ mask, long n, int mode, int vec, long nc,
         const FgCtl* __restrict__ ctl, double q_lo, double q_hi, double* __restrict__ psum, double* __restrict__ psq,
         uint32_t* __restrict__ pkmin, uint32_t* __restrict__ pkmax, uint32_t* __restrict__ pab0, uint32_t* __restrict__ pab1) {
  __shared__ uint32_t s_scan[8];
  const int m = threadIdx.x & 63;
  const long chunk = (long)blockIdx.x * kSumChunks + (threadIdx.x >> 6);
  const long base = chunk * kMskRedChunk;
  const bool active = chunk < nc;                        // uniform over a wavefront
  const bool whole = active && vec && n - base >= kMskRedChunk;
  const bool use_mask = mode == MSK_MASK_LABEL;
  float4 v[16];
  if (whole) {                                           // in flight while the histograms are read and scanned
    const float4* x4 = reinterpret_cast<const float4*>(x + base);
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = x4[64 * j + m];
  }
  const FgSel fs = fg_resolve<kMskSelPasses>(ctl, q_lo, q_hi, s_scan);
  if (fs.nv == 0) return;                                // uniform; the finish pass does not read the chunk values then
  if (!active) return;                                   // behind the last barrier
  const uint32_t akey0 = fs.sel[0].prefix, akey1 = fs.sel[1].prefix;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
  uint32_t kmin = kNoKey, kmax = 0u, ab0 = kNoKey, ab1 = kNoKey;
  auto add = [&](int i, float f, int32_t mk, bool inside) {
    double d = 0.0;
    if (inside && fg_valid(mode, f, mk)) {
      d = (double)f;
      const uint32_t key = msk_sel_key(f);
      kmin = key < kmin ? key : kmin;
      kmax = key > kmax ? key : kmax;
      if (key > akey0 && key < ab0) ab0 = key;
      if (key > akey1 && key < ab1) ab1 = key;
    }
    s[i] = s[i] + d;                                     // an invalid voxel and one past n add the statement's + 0.0
    q[i] = q[i] + d * d;
  };
  if (whole) {
    const int4* m4 = reinterpret_cast<const int4*>(mask + (use_mask ? base : 0));
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      int4 mk = make_int4(1, 1, 1, 1);
      if (use_mask) mk = m4[64 * j + m];
      add(0, v[j].x, mk.x, true); add(1, v[j].y, mk.y, true); add(2, v[j].z, mk.z, true); add(3, v[j].w, mk.w, true);
    }
  } else {
    const long left = n - base;
    for (int j = 0; j < 16; ++j) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long e = 256L * j + 4 * m + i;
        const bool inside = e < left;
        add(i, inside ? x[base + e] : 0.f, (inside && use_mask) ? mask[base + e] : 1, inside);
      }
    }
  }
  const double cs = msk_red_chunk_tree(s), cq = msk_red_chunk_tree(q);
  kmin = fg_wave_min_u32(kmin);
  kmax = fg_wave_max_u32(kmax);
  ab0 = fg_wave_min_u32(ab0);
  ab1 = fg_wave_min_u32(ab1);
  if (m == 0) {
    psum[chunk] = cs;
    psq[chunk] = cq;
    pkmin[chunk] = kmin;
    pkmax[chunk] = kmax;
    pab0[chunk] = ab0;
    pab1[chunk] = ab1;
  }
}

// one percentile from its rank, the selected key a = s[i], the keys above it and the smallest of them
__device__ __forceinline__ void fg_percentile(const FgRank& r, const msk_sel& sel, uint32_t nv, uint32_t above_key, double* p,
                                              double* a_out, double* b_out) {
  const double a = (double)msk_sel_unkey(sel.prefix);
  // ranks [nv - ngt - neq, nv - ngt) hold a; s[i + 1] is a as long as i + 1 stays among them (or i is the last rank)
  const bool b_is_a = sel.ngt == 0u || (unsigned long long)r.i + 1ull + sel.ngt < (unsigned long long)nv;
  const double b = b_is_a ? a : (double)msk_sel_unkey(above_key);
  const double d = b - a;
  double res;
  if (r.g >= 0.5) {
    const double t = d * (1.0 - r.g);
    res = b - t;
  } else {
    const double t = d * r.g;
    res = a + t;
  }
  *p = res;
  *a_out = a;
  *b_out = b;
}

// one workgroup of 256; thread 0 writes the record
__global__ void __launch_bounds__(kMskRedLanes)
fg_finish_k(long nc, const FgCtl* __restrict__ ctl, double q_lo, double q_hi, const double* __restrict__ psum,
            const double* __restrict__ psq, const uint32_t* __restrict__ pkmin, const uint32_t* __restrict__ pkmax,
            const uint32_t* __restrict__ pab0, const uint32_t* __restrict__ pab1, double* __restrict__ rec) {
  __shared__ uint32_t s_scan[8];
  __shared__ uint32_t s_k[4][kMskRedLanes / 64];
  const FgSel fs = fg_resolve<kMskSelPasses>(ctl, q_lo, q_hi, s_scan);
  if (fs.nv == 0) {
    if (threadIdx.x < 16) rec[threadIdx.x] = 0.0;
    return;
  }
  const double sum = msk_red_finish<false>(nc, nullptr, psum, nullptr, nullptr).sumsq;   // the ordered sum of the chunk values
  __syncthreads();
  const double sumsq = msk_red_finish<false>(nc, nullptr, psq, nullptr, nullptr).sumsq;
  uint32_t kmin = kNoKey, kmax = 0u, ab0 = kNoKey, ab1 = kNoKey;
  for (long c = threadIdx.x; c < nc; c += kMskRedLanes) {
    const uint32_t a = pkmin[c], b = pkmax[c], c0 = pab0[c], c1 = pab1[c];
    kmin = a < kmin ? a : kmin;
    kmax = b > kmax ? b : kmax;
    ab0 = c0 < ab0 ? c0 : ab0;
    ab1 = c1 < ab1 ? c1 : ab1;
  }
  kmin = fg_wave_min_u32(kmin);
  kmax = fg_wave_max_u32(kmax);
  ab0 = fg_wave_min_u32(ab0);
  ab1 = fg_wave_min_u32(ab1);
  if ((threadIdx.x & 63) == 0) {
    const int wv = threadIdx.x >> 6;
    s_k[0][wv] = kmin; s_k[1][wv] = kmax; s_k[2][wv] = ab0; s_k[3][wv] = ab1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int wv = 1; wv < kMskRedLanes / 64; ++wv) {
      kmin = s_k[0][wv] < kmin ? s_k[0][wv] : kmin;
      kmax = s_k[1][wv] > kmax ? s_k[1][wv] : kmax;
      ab0 = s_k[2][wv] < ab0 ? s_k[2][wv] : ab0;
      ab1 = s_k[3][wv] < ab1 ? s_k[3][wv] : ab1;
    }
    const double nvd = (double)fs.nv;
    const double mean = sum / nvd;
    const double e2 = sumsq / nvd;
    const double mm = mean * mean;
    double var = e2 - mm;
    var = var > 0.0 ? var : 0.0;
    double p[kRanks], a[kRanks], b[kRanks];
    fg_percentile(fs.rank[0], fs.sel[0], fs.nv, ab0, &p[0], &a[0], &b[0]);
    fg_percentile(fs.rank[1], fs.sel[1], fs.nv, ab1, &p[1], &a[1], &b[1]);
    rec[0] = nvd;
    rec[1] = (double)msk_sel_unkey(kmin);
    rec[2] = (double)msk_sel_unkey(kmax);
    rec[3] = sum;
    rec[4] = sumsq;
    rec[5] = mean;
    rec[6] = sqrt(var);
    rec[7] = p[0];
    rec[8] = p[1];
    rec[9] = a[0];
    rec[10] = b[0];
    rec[11] = fs.rank[0].g;
    rec[12] = a[1];
    rec[13] = b[1];
    rec[14] = fs.rank[1].g;
    rec[15] = 0.0;
  }
}

// ---- the apply pass ----------------------------------------------------------------------------------------------------------
struct NormArgs {
  long n;
  int mode, flags;
  float outside;
  float lo, hi, m, inv;          // from the host's four doubles; a device record replaces them
};

struct NormOp {
  float lo, hi, m, inv, outside;
  int mode;
  bool clip, zscore, mask_out;

  __device__ __forceinline__ NormOp(const NormArgs& g, const double* __restrict__ rec)
      : lo(g.lo), hi(g.hi), m(g.m), inv(g.inv), outside(g.outside), mode(g.mode), clip((g.flags & MSK_NORM_CLIP) != 0),
        zscore((g.flags & MSK_NORM_ZSCORE) != 0), mask_out((g.flags & MSK_NORM_MASK_OUT) != 0) {
    if (rec != nullptr) {
      const double sd = rec[6];
      lo = (float)rec[7];
      hi = (float)rec[8];
      m = (float)rec[5];
      inv = (float)(1.0 / (sd > 1e-8 ? sd : 1e-8));
    }
  }
  __device__ __forceinline__ float operator()(float x, int32_t mk) const {
    float c = x;
    if (clip) {
      c = c < lo ? lo : c;
      c = c > hi ? hi : c;
    }
    if (zscore) c = (c - m) * inv;
    if (mask_out && !fg_valid(mode, x, mk)) c = outside;
    return c;
  }
};

// tiles of 1024 quads per workgroup, grid-stride; then the n % 4 tail (first workgroup).  The first tile's loads go out before
// the record is read (the forward pass's last store: the lesson of msk_sgd_momentum_clip).
__global__ void __launch_bounds__(kThreads)
clip_zscore_vec_k(const float* __restrict__ x, const int32_t* __restrict__ mask, float* __restrict__ y, const NormArgs g,
                  const double* __restrict__ rec) {
  const long nq = g.n >> 2;
  const bool use_mask = mask != nullptr;                 // null unless the mask decides something
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const int4* m4 = reinterpret_cast<const int4*>(mask);
  float4* y4 = reinterpret_cast<float4*>(y);
  long t0 = (long)blockIdx.x * 1024;
  float4 v[4];
  int4 mk[4];
  auto load = [&](long t) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long qi = t + k * kThreads + threadIdx.x;
      mk[k] = make_int4(1, 1, 1, 1);
      if (qi < nq) {
        v[k] = x4[qi];
        if (use_mask) mk[k] = m4[qi];
      }
    }
  };
  if (t0 < nq) load(t0);
  const NormOp op(g, rec);
  while (t0 < nq) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long qi = t0 + k * kThreads + threadIdx.x;
      if (qi < nq) {
        float4 r;
        r.x = op(v[k].x, mk[k].x);
        r.y = op(v[k].y, mk[k].y);
        r.z = op(v[k].z, mk[k].z);
        r.w = op(v[k].w, mk[k].w);
        y4[qi] = r;
      }
    }
    t0 += (long)gridDim.x * 1024;
    if (t0 < nq) load(t0);
  }
  if (blockIdx.x == 0) {
    const long i = 4 * nq + threadIdx.x;
    if (threadIdx.x < 4 && i < g.n) y[i] = op(x[i], use_mask ? mask[i] : 1);
  }
}

__global__ void __launch_bounds__(kThreads)
clip_zscore_elem_k(const float* __restrict__ x, const int32_t* __restrict__ mask, float* __restrict__ y, const NormArgs g,
                   const double* __restrict__ rec) {
  const long stride = (long)gridDim.x * kThreads;
  long i = (long)blockIdx.x * kThreads + threadIdx.x;
  float f = 0.f;
  int32_t mk = 1;
  if (i < g.n) {
    f = x[i];
    if (mask != nullptr) mk = mask[i];
  }
  const NormOp op(g, rec);
  while (i < g.n) {
    const float r = op(f, mk);
    const long at = i;
    i += stride;
    if (i < g.n) {
      f = x[i];
      if (mask != nullptr) mk = mask[i];
    }
    y[at] = r;
  }
}

// ---- the bounding box --------------------------------------------------------------------------------------------------------
// box while the pass runs: {D - d0, H - h0, W - w0, d1, h1, w1, count, 0}, all under atomicMax / atomicAdd from zero
__global__ void __launch_bounds__(kThreads)
nonzero_bbox_k(const uint32_t* __restrict__ src, long n, uint32_t H, uint32_t W, uint32_t keep, int vec, int32_t* __restrict__ box) {
  __shared__ int s_r[7][kThreads / 64];
  const long stride = (long)gridDim.x * kThreads;
  int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {-1, -1, -1};
  uint32_t cnt = 0;
  auto see = [&](uint32_t bits, uint32_t d, uint32_t h, uint32_t w) {
    if ((bits & keep) != 0u) {
      ++cnt;
      mn[0] = min(mn[0], (int)d); mx[0] = max(mx[0], (int)d);
      mn[1] = min(mn[1], (int)h); mx[1] = max(mx[1], (int)h);
      mn[2] = min(mn[2], (int)w); mx[2] = max(mx[2], (int)w);
    }
  };
  auto split = [&](uint32_t e, uint32_t& d, uint32_t& h, uint32_t& w) {   // e < 2^31
    const uint32_t row = e / W;
    w = e - row * W;
    d = row / H;
    h = row - d * H;
  };
  if (vec) {
    const long n4 = n >> 2;
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    // tiles of 1024 quads per workgroup: a thread's four loads are issued together
    for (long t0 = (long)blockIdx.x * 1024; t0 < n4; t0 += (long)gridDim.x * 1024) {
      uint4 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long qi = t0 + k * kThreads + threadIdx.x;
        v[k] = qi < n4 ? s4[qi] : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (((v[k].x | v[k].y | v[k].z | v[k].w) & keep) == 0u) continue;   // -0.0 | bits of a non-zero stays non-zero: exact
        const long qi = t0 + k * kThreads + threadIdx.x;
        uint32_t d, h, w;
        split((uint32_t)(4 * qi), d, h, w);
        const uint32_t e4[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          see(e4[j], d, h, w);
          if (++w == W) {
            w = 0;
            if (++h == H) { h = 0; ++d; }
          }
        }
      }
    }
    if (blockIdx.x == 0) {
      const long e = 4 * n4 + threadIdx.x;
      if (threadIdx.x < 4 && e < n) {
        uint32_t d, h, w;
        split((uint32_t)e, d, h, w);
        see(src[e], d, h, w);
      }
    }
  } else {
    for (long e = (long)blockIdx.x * kThreads + threadIdx.x; e < n; e += stride) {
      const uint32_t b = src[e];
      if ((b & keep) == 0u) continue;
      uint32_t d, h, w;
      split((uint32_t)e, d, h, w);
      see(b, d, h, w);
    }
  }
  int r[7] = {mn[0], mn[1], mn[2], mx[0], mx[1], mx[2], (int)cnt};
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = min(r[k], __shfl_xor(r[k], o, 64));
#pragma unroll
    for (int k = 3; k < 6; ++k) r[k] = max(r[k], __shfl_xor(r[k], o, 64));
    r[6] += __shfl_xor(r[6], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) s_r[k][threadIdx.x >> 6] = r[k];
  }
  __syncthreads();
  if (threadIdx.x < 7) {                                 // one value and at most one atomic per thread
    const int k = threadIdx.x;
    int acc = s_r[k][0];
    for (int wv = 1; wv < kThreads / 64; ++wv) {
      const int t = s_r[k][wv];
      acc = k < 3 ? min(acc, t) : (k < 6 ? max(acc, t) : acc + t);
    }
    int total = s_r[6][0];
    for (int wv = 1; wv < kThreads / 64; ++wv) total += s_r[6][wv];
    if (total > 0) {                                     // a workgroup that saw nothing issues nothing
      if (k < 6) {
        // an extreme is sent only if it moves the record: the word only grows from the memset's zero, so whatever value this
        // agent-scope load returns is no larger than the word is, and a stale one costs an atomic, never a result
        const int ext = k == 0 ? (int)(n / ((long)H * W)) : (k == 1 ? (int)H : (int)W);
        const int val = k < 3 ? ext - acc : acc + 1;
        if (val > __hip_atomic_load(&box[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&box[k], val);
      } else {
        atomicAdd(&box[6], acc);
      }
    }
  }
}

__global__ void nonzero_bbox_finish_k(int D, int H, int W, int32_t* __restrict__ box) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && box[6] > 0) {
    box[0] = D - box[0];
    box[1] = H - box[1];
    box[2] = W - box[2];
  }
}

inline bool fg_mode_ok(int mode) { return mode == MSK_MASK_ALL || mode == MSK_MASK_NONZERO || mode == MSK_MASK_LABEL; }

}  // namespace

extern "C" {

int msk_fg_stats_workspace(long n, size_t* bytes) {
  MSK_REQUIRE(nullptr, bytes != nullptr, "bytes must not be null");
  MSK_REQUIRE(nullptr, n >= 1 && n <= 0x7fffffffL, "n must be in [1, 2^31)");
  *bytes = fg_ws_bytes(n);
  return 0;
}

int msk_fg_stats(msk_ctx* ctx, const float* x, const int32_t* mask, long n, int mask_mode, double q_lo, double q_hi, void* workspace,
                 double* record) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, x != nullptr && workspace != nullptr && record != nullptr, "null x / workspace / record");
  MSK_REQUIRE(ctx, n >= 1 && n <= 0x7fffffffL, "n must be in [1, 2^31)");
  MSK_REQUIRE(ctx, fg_mode_ok(mask_mode), "mask_mode must be one of MSK_MASK_*");
  MSK_REQUIRE(ctx, mask_mode != MSK_MASK_LABEL || mask != nullptr, "MSK_MASK_LABEL needs a mask");
  MSK_REQUIRE(ctx, q_lo >= 0.0 && q_hi <= 100.0 && q_lo <= q_hi, "percentiles must satisfy 0 <= q_lo <= q_hi <= 100");
  MSK_REQUIRE(ctx, ((((uintptr_t)x) | ((uintptr_t)mask)) & 3) == 0, "x / mask must be 4-byte aligned");
  MSK_REQUIRE(ctx, (((uintptr_t)workspace) & 15) == 0 && (((uintptr_t)record) & 7) == 0,
              "workspace must be 16-byte, record 8-byte aligned");
  const size_t wb = fg_ws_bytes(n);
  MSK_REQUIRE(ctx, msk_bytes_disjoint(workspace, wb, x, (size_t)n * 4) && msk_bytes_disjoint(workspace, wb, record, 128) &&
                       (mask == nullptr || msk_bytes_disjoint(workspace, wb, mask, (size_t)n * 4)),
              "workspace overlaps an operand");
  MSK_REQUIRE(ctx, msk_bytes_disjoint(record, 128, x, (size_t)n * 4) &&
                       (mask == nullptr || msk_bytes_disjoint(record, 128, mask, (size_t)n * 4)),
              "record overlaps an operand");
  const FgWs ws = fg_ws(workspace, n);
  const int32_t* mk = mask_mode == MSK_MASK_LABEL ? mask : nullptr;
  MSK_CHECK_HIP(ctx, hipMemsetAsync(ws.ctl, 0, sizeof(FgCtl), ctx->stream));
  const int vec = ((((uintptr_t)x) | ((uintptr_t)mk)) & 15) == 0;
  const int nb = msk_ew_blocks(vec ? (n + 3) / 4 : n, ctx->num_cu, 2);
  {
    msk_launch_scope ls(ctx, "fg_hist");
    hipLaunchKernelGGL((fg_hist_k<0>), dim3(nb), dim3(kThreads), 0, ctx->stream, x, mk, n, mask_mode, vec, ws.ctl, q_lo, q_hi);
    hipLaunchKernelGGL((fg_hist_k<1>), dim3(nb), dim3(kThreads), 0, ctx->stream, x, mk, n, mask_mode, vec, ws.ctl, q_lo, q_hi);
    hipLaunchKernelGGL((fg_hist_k<2>), dim3(nb), dim3(kThreads), 0, ctx->stream, x, mk, n, mask_mode, vec, ws.ctl, q_lo, q_hi);
    MSK_LAUNCH_CHECK(ctx);
  }
  const long nc = msk_chunks_of((size_t)n);
  {
    msk_launch_scope ls(ctx, "fg_sum");
    hipLaunchKernelGGL(fg_sum_k, dim3((unsigned)((nc + kSumChunks - 1) / kSumChunks)), dim3(kThreads), 0, ctx->stream, x, mk, n,
                       mask_mode, vec, nc, (const FgCtl*)ws.ctl, q_lo, q_hi, ws.psum, ws.psq, ws.kmin, ws.kmax, ws.above[0],
                       ws.above[1]);
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "fg_finish");
    hipLaunchKernelGGL(fg_finish_k, dim3(1), dim3(kMskRedLanes), 0, ctx->stream, nc, (const FgCtl*)ws.ctl, q_lo, q_hi,
                       (const double*)ws.psum, (const double*)ws.psq, (const uint32_t*)ws.kmin, (const uint32_t*)ws.kmax,
                       (const uint32_t*)ws.above[0], (const uint32_t*)ws.above[1], record);
    MSK_LAUNCH_CHECK(ctx);
  }
  return 0;
}

int msk_clip_zscore(msk_ctx* ctx, const float* x, const int32_t* mask, long n, int mask_mode, const double* record,
                    const double* host_params, int flags, float outside, float* y) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, x != nullptr && y != nullptr, "null x / y");
  MSK_REQUIRE(ctx, record != nullptr || host_params != nullptr, "a device record or four host doubles must be given");
  MSK_REQUIRE(ctx, n >= 1 && n <= 0x7fffffffL, "n must be in [1, 2^31)");
  MSK_REQUIRE(ctx, fg_mode_ok(mask_mode), "mask_mode must be one of MSK_MASK_*");
  MSK_REQUIRE(ctx, (flags & ~(MSK_NORM_CLIP | MSK_NORM_ZSCORE | MSK_NORM_MASK_OUT)) == 0, "flags must be a combination of MSK_NORM_*");
  MSK_REQUIRE(ctx, mask_mode != MSK_MASK_LABEL || mask != nullptr, "MSK_MASK_LABEL needs a mask");
  MSK_REQUIRE(ctx, ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)mask)) & 3) == 0, "x / y / mask must be 4-byte aligned");
  MSK_REQUIRE(ctx, (((uintptr_t)record) & 7) == 0, "record must be 8-byte aligned");
  const size_t bytes = (size_t)n * 4;
  MSK_REQUIRE(ctx, (const float*)y == x || msk_bytes_disjoint(x, bytes, y, bytes), "y must be x or not overlap it");
  MSK_REQUIRE(ctx, (mask == nullptr || msk_bytes_disjoint(mask, bytes, y, bytes)) &&
                       (record == nullptr || msk_bytes_disjoint(record, 128, y, bytes)),
              "y must overlap neither mask nor record");
  NormArgs g;
  g.n = n;
  g.mode = mask_mode;
  g.flags = flags;
  g.outside = outside;
  g.lo = g.hi = g.m = 0.f;
  g.inv = 1.f;
  if (record == nullptr) {
    const double sd = host_params[3];
    g.lo = (float)host_params[0];
    g.hi = (float)host_params[1];
    g.m = (float)host_params[2];
    g.inv = (float)(1.0 / (sd > 1e-8 ? sd : 1e-8));
  }
  // the mask is read only where it decides something
  const int32_t* mk = (mask_mode == MSK_MASK_LABEL && (flags & MSK_NORM_MASK_OUT)) ? mask : nullptr;
  const bool vec = ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)mk)) & 15) == 0 && n >= 4;
  const long cap = (long)ctx->num_cu * 8;
  msk_launch_scope ls(ctx, "clip_zscore");
  if (vec) {
    const long tiles = ((n >> 2) + 1023) / 1024;
    hipLaunchKernelGGL(clip_zscore_vec_k, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(kThreads), 0, ctx->stream, x, mk, y, g,
                       record);
  } else {
    const long blocks = (n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(clip_zscore_elem_k, dim3((unsigned)(blocks < 4 * cap ? blocks : 4 * cap)), dim3(kThreads), 0, ctx->stream, x,
                       mk, y, g, record);
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

int msk_nonzero_bbox(msk_ctx* ctx, const void* src, int d, int h, int w, int dtype, int32_t* box) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, src != nullptr && box != nullptr, "null src / box");
  MSK_REQUIRE(ctx, d >= 1 && h >= 1 && w >= 1, "extents must be >= 1");
  MSK_REQUIRE(ctx, msk_below_2_31(d, h, w), "the volume must have fewer than 2^31 voxels");
  MSK_REQUIRE(ctx, dtype == 0 || dtype == 1, "dtype must be 0 (float32) or 1 (int32)");
  MSK_REQUIRE(ctx, ((((uintptr_t)src) | ((uintptr_t)box)) & 3) == 0, "src / box must be 4-byte aligned");
  const long n = (long)d * h * w;
  MSK_REQUIRE(ctx, msk_bytes_disjoint(box, 32, src, (size_t)n * 4), "box overlaps the volume");
  MSK_CHECK_HIP(ctx, hipMemsetAsync(box, 0, 32, ctx->stream));
  const int vec = (((uintptr_t)src) & 15) == 0;
  const uint32_t keep = dtype == 0 ? 0x7fffffffu : 0xffffffffu;   // float32: everything but the sign bit, so -0.0 is zero and a NaN is not
  msk_launch_scope ls(ctx, "nonzero_bbox");
  // vec: a workgroup per tile of 1024 quads, at most 4 per CU (every workgroup that saw a voxel adds to the count word)
  hipLaunchKernelGGL(nonzero_bbox_k, dim3(msk_ew_blocks(vec ? (n + 15) / 16 : n, ctx->num_cu, 4)), dim3(kThreads), 0, ctx->stream,
                     (const uint32_t*)src, n, (uint32_t)h, (uint32_t)w, keep, vec, box);
  hipLaunchKernelGGL(nonzero_bbox_finish_k, dim3(1), dim3(64), 0, ctx->stream, d, h, w, box);
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
