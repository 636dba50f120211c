// Device and launch helpers shared by the libmsegk translation units (gfx950 only); included by msk_common.h.  Whatever two
// kernel files need alike is stated HERE once: the pieces with a bit-for-bit contract against a numpy statement under tests/
// (the fixed-order float64 reduction: tests/clip_reference.py, tests/intensity_reference.py) above all.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "msegk.h"

// ---- grid size and argument predicates (host) ----------------------------------------------------------------------------------
// workgroups of 256 threads for a grid-stride kernel over `total` items: clamp(ceil(total / 256), 1, num_cu * per_cu)
static inline int msk_ew_blocks(long total, int num_cu, int per_cu = 16) {
  long b = (total + 255) / 256;
  const long cap = (long)num_cu * per_cu;
  if (b > cap) b = cap;
  return (int)(b < 1 ? 1 : b);
}

static inline bool msk_well_formed(const msk_tensor& t) {   // a non-empty float tensor with ld >= c
  return t.p != nullptr && (((uintptr_t)t.p) & 3) == 0 && t.n >= 1 && t.d >= 1 && t.h >= 1 && t.w >= 1 && t.c >= 1 && t.ld >= t.c;
}
static inline bool msk_quad_dense(const msk_tensor& t) { return t.ld == t.c && (((uintptr_t)t.p) & 15) == 0; }
static inline bool msk_same_shape(const msk_tensor& a, const msk_tensor& b) {
  return a.n == b.n && a.d == b.d && a.h == b.h && a.w == b.w && a.c == b.c;
}
static inline bool msk_below_2_31(int d, int h, int w) { return (long)d * h * w <= 0x7fffffffL; }
static inline bool msk_bytes_disjoint(const void* a, size_t abytes, const void* b, size_t bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 + abytes <= b0 || b0 + bbytes <= a0;
}

// ---- LDS tiles, the counter RNG's word, wavefront sums ---------------------------------------------------------------------------
// Dense voxel records of rq float4 quads (rq <= 8) between HBM and an LDS tile of 256 records with WHOLE-LINE accesses (round 4):
// a thread-per-voxel kernel whose lane reads its own 80-byte record touches 40 lines per 1 KiB load instruction and ran at
// 1-1.9 TB/s (the 20-class MRI head and its loss: pointwise_mid_k, loss_*_tpv_k); here consecutive lanes move consecutive
// 16-byte quads and a thread then takes its record from LDS.  pitch = rq | 1 slots: 16 consecutive records sit on 16 distinct
// 16-byte bank groups, so the per-record ds_read_b128 / ds_write_b128 are conflict-free.
__device__ __forceinline__ void msk_tile_load(const float* __restrict__ src, int nquads, int rq, int pitch, float4* __restrict__ tile) {
  const float4* s4 = reinterpret_cast<const float4*>(src);
  for (int i = threadIdx.x; i < nquads; i += blockDim.x) {
    const int v = i / rq, q = i - v * rq;
    tile[v * pitch + q] = s4[i];
  }
}
__device__ __forceinline__ void msk_tile_store(float* __restrict__ dst, int nquads, int rq, int pitch, const float4* __restrict__ tile, bool accumulate) {
  float4* d4 = reinterpret_cast<float4*>(dst);
  for (int i = threadIdx.x; i < nquads; i += blockDim.x) {
    const int v = i / rq, q = i - v * rq;
    float4 r = tile[v * pitch + q];
    if (accumulate) {
      const float4 o = d4[i];
      r.x += o.x; r.y += o.y; r.z += o.z; r.w += o.w;
    }
    d4[i] = r;
  }
}

// flat form of msk_tile_load for records that are not whole quads (3 classes: 12 bytes): the tile's floats are copied as they
// lie (16-byte accesses, scalar tail), a thread's record starts at float tid * C -- an odd stride for C = 3: conflict-free
// (the loss kernels of msk_loss_optim.hip and msk_loss_region.hip)
__device__ __forceinline__ void tile_load_flat(const float* __restrict__ src, int nfloats, float* __restrict__ tile) {
  const int nq = nfloats >> 2;
  for (int i = threadIdx.x; i < nq; i += blockDim.x) reinterpret_cast<float4*>(tile)[i] = reinterpret_cast<const float4*>(src)[i];
  for (int i = 4 * nq + threadIdx.x; i < nfloats; i += blockDim.x) tile[i] = src[i];
}
__device__ __forceinline__ void tile_store_flat(float* __restrict__ dst, int nfloats, const float* __restrict__ tile) {
  const int nq = nfloats >> 2;
  for (int i = threadIdx.x; i < nq; i += blockDim.x) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(tile)[i];
  for (int i = 4 * nq + threadIdx.x; i < nfloats; i += blockDim.x) dst[i] = tile[i];
}
// tile_store_flat adding into dst
__device__ __forceinline__ void tile_add_flat(float* __restrict__ dst, int nfloats, const float* __restrict__ tile) {
  const int nq = nfloats >> 2;
  for (int i = threadIdx.x; i < nq; i += blockDim.x) {
    float4 r = reinterpret_cast<const float4*>(tile)[i];
    const float4 o = reinterpret_cast<float4*>(dst)[i];
    r.x += o.x; r.y += o.y; r.z += o.z; r.w += o.w;
    reinterpret_cast<float4*>(dst)[i] = r;
  }
  for (int i = 4 * nq + threadIdx.x; i < nfloats; i += blockDim.x) dst[i] += tile[i];
}

// ---- the thread-per-voxel scaffold of the loss kernels ----------------------------------------------------------------------------
// loss_stats_tpv_k / loss_bwd_tpv_k (msk_loss_optim.hip) and region_stats_k / region_bwd_k (msk_loss_region.hip): a thread owns a
// voxel, its C <= CM logits sit in registers (CM: the class count rounded up in steps of a quad), a workgroup of kTpvThreads takes
// tiles of kTpvThreads consecutive voxels, and the gradient record goes back the way the logits came.  The lane-per-class
// kernels this form replaced for C > 4 spent two 32-lane shuffle reductions per voxel and left 12 of 32 lanes idle: 0.45 +
// 0.49 ms per output of the 20-class MRI model at 512 x 512 x 12, four outputs with deep supervision.  ST is the way a record
// travels:
//   ST = 1  (round 4) dense logits (ld == C, C % 4 == 0) go through an LDS tile of 256 voxel records with whole-line accesses
//           (msk_tile_load) -- a lane reading its own 80-byte record straight from HBM held these passes at 1.0 / 1.9 TB/s;
//   ST = 2  the flat form for dense C <= 4 (tile_load_flat): the 3-class head of the lung model ran the lane-per-class kernels
//           (four lanes per voxel, one idle, 192 bytes per load instruction: 60 + 67 us per step at 2 x 128^3);
//   ST = 0  a lane's own loads and stores for channel-slice views (ld > C), unaligned pointers and everything else.
// Only the movement is shared: every kernel keeps its own arithmetic, whose order is part of its result.  And a kernel takes a
// piece only where the call leaves its registers, LDS and instruction stream (read in the assembly, register names aside) what
// its own text gave.  That is: the tile size and the ladder everywhere; the fill in loss_stats_tpv_k, loss_bwd_tpv_k and
// region_stats_k; the take in both region kernels; the store of the tile forms in region_bwd_k.  Through the other calls the
// compiler scheduled the kernel differently: the take split loss_stats_tpv_k's wait for its arguments in two and, with a shared
// block reduction, cost 0.4 us per launch at 3 classes; take and store moved loss_bwd_tpv_k's tuned register counts, the fill
// region_bwd_k<12, 0>'s; a shared ST = 0 store and a shared block reduction reordered the region kernels.
constexpr int kTpvThreads = 256;

constexpr int tpv_pitch(int CM) { return (CM / 4) | 1; }   // quads between two records of the ST = 1 tile
constexpr int tpv_tile_quads(int CM, int ST) { return ST == 1 ? kTpvThreads * tpv_pitch(CM) : (ST == 2 ? kTpvThreads * CM / 4 : 1); }

// the nv records from src = the tile's first logit into the LDS tile, between two barriers (the first: the previous round's
// reads or store pass of the tile are over).  Reached by every thread of the workgroup; ST = 0: nothing.
template <int CM, int ST>
__device__ __forceinline__ void tpv_fill(float4* __restrict__ tile, const float* __restrict__ src, int nv, int C) {
  if (ST) {
    __syncthreads();
    if (ST == 2) tile_load_flat(src, nv * C, reinterpret_cast<float*>(tile));
    else msk_tile_load(src, nv * (C >> 2), C >> 2, tpv_pitch(CM), tile);
    __syncthreads();
  }
}

// this thread's record into zz[0..C), zz[C..CM) = 0: from the tile (ST = 2, 1) or from zp = its first logit in memory (ST = 0,
// element by element).  Only for a thread that has a voxel.
template <int CM, int ST>
__device__ __forceinline__ void tpv_take(float (&zz)[CM], const float4* __restrict__ tile, const float* __restrict__ zp, int C) {
  if (ST == 2) {
#pragma unroll
    for (int c = 0; c < CM; ++c) zz[c] = c < C ? reinterpret_cast<const float*>(tile)[threadIdx.x * C + c] : 0.f;
  } else if (ST == 1) {
#pragma unroll
    for (int c = 0; c < CM; c += 4) {
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < C) q = tile[threadIdx.x * tpv_pitch(CM) + (c >> 2)];
      zz[c] = q.x; zz[c + 1] = q.y; zz[c + 2] = q.z; zz[c + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < CM; ++c) zz[c] = c < C ? zp[c] : 0.f;
  }
}

// the gradient records back through the tile (reached by every thread): barrier (every thread has taken its record), the threads
// with `mine` write g into the tile, barrier, the tile's nv records go to dz_tile = the tile's first gradient, added to what is
// there with `accumulate`.  A record that no thread wrote is never stored (nv ends before it).  ST = 0: nothing, the caller
// stores its own voxel's record.
template <int CM, int ST>
__device__ __forceinline__ void tpv_put(const float (&g)[CM], float4* __restrict__ tile, float* __restrict__ dz_tile,
                                        int C, int nv, bool mine, bool accumulate) {
  if (ST == 2) {
    __syncthreads();
    if (mine) {
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) reinterpret_cast<float*>(tile)[threadIdx.x * C + c] = g[c];
    }
    __syncthreads();
    if (accumulate) tile_add_flat(dz_tile, nv * C, reinterpret_cast<const float*>(tile));
    else tile_store_flat(dz_tile, nv * C, reinterpret_cast<const float*>(tile));
  } else if (ST == 1) {
    __syncthreads();
    if (mine) {
#pragma unroll
      for (int c = 0; c < CM; c += 4)
        if (c < C) tile[threadIdx.x * tpv_pitch(CM) + (c >> 2)] = make_float4(g[c], g[c + 1], g[c + 2], g[c + 3]);
    }
    __syncthreads();
    msk_tile_store(dz_tile, nv * (C >> 2), C >> 2, tpv_pitch(CM), tile, accumulate);
  }
}

// the CM ladder: LAUNCH(CM, ST) for 4 < C <= 32 with the register arrays sized to the class count in steps of a quad (round 4:
// 20 classes ran the 32-slot instantiation), ST = 1 where QUAD holds and 0 otherwise.  What goes to the ladder, and the forms
// outside it (C <= 4, C > 32), is each file's own decision.
#define MSK_TPV_LADDER(C_, QUAD_, LAUNCH)                    \
  do {                                                       \
    if ((C_) <= 8) { MSK_TPV_STEP(8, QUAD_, LAUNCH) }        \
    else if ((C_) <= 12) { MSK_TPV_STEP(12, QUAD_, LAUNCH) } \
    else if ((C_) <= 16) { MSK_TPV_STEP(16, QUAD_, LAUNCH) } \
    else if ((C_) <= 20) { MSK_TPV_STEP(20, QUAD_, LAUNCH) } \
    else if ((C_) <= 24) { MSK_TPV_STEP(24, QUAD_, LAUNCH) } \
    else { MSK_TPV_STEP(32, QUAD_, LAUNCH) }                 \
  } while (0)
#define MSK_TPV_STEP(CM_, QUAD_, LAUNCH) if (QUAD_) LAUNCH(CM_, 1); else LAUNCH(CM_, 0);

// splitmix64: the word of the counter RNGs (Dropout3D masks in msk_elementwise.hip, Gaussian noise in msk_intensity.hip)
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ float msk_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ double msk_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t msk_wave_sum_u32(uint32_t v) {   // the sum in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- scans over a wavefront and a workgroup ----------------------------------------------------------------------------------------
struct msk_op_add { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct msk_op_max { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };
struct msk_op_min { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; } };

// Inclusive scan of one value per lane in lane order (REV: in reverse lane order, i.e. over the lanes behind this one).
template <bool REV, class Op>
__device__ __forceinline__ uint32_t msk_wave_incl_scan(uint32_t v, Op op) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int src = REV ? lane + o : lane - o;
    const uint32_t t = __shfl(v, src & 63, 64);
    if (src >= 0 && src < 64) v = op(v, t);
  }
  return v;
}

// Exclusive scan of one value per thread in thread order (REV: in reverse thread order, i.e. over the threads behind this
// one); *total = the combination of all threads.  Called by every thread.  wtot: one LDS word per wavefront, reusable after the
// call returns.
template <bool REV, class Op>
__device__ __forceinline__ uint32_t msk_block_excl_scan(uint32_t v, uint32_t identity, Op op, uint32_t* wtot, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint32_t inc = msk_wave_incl_scan<REV>(v, op);
  const int nb = REV ? lane + 1 : lane - 1;
  const uint32_t left = __shfl(inc, nb & 63, 64);
  uint32_t ex = (nb >= 0 && nb < 64) ? left : identity;
  __syncthreads();   // the previous use of wtot is over
  if (lane == (REV ? 0 : 63)) wtot[wave] = inc;
  __syncthreads();
  uint32_t before = identity, all = identity;
  for (int w = 0; w < nw; ++w) {
    const uint32_t t = wtot[w];
    all = op(all, t);
    if (REV ? w > wave : w < wave) before = op(before, t);
  }
  *total = all;
  return op(before, ex);
}
template <bool REV, class Op>
__device__ __forceinline__ uint32_t msk_block_excl_scan(uint32_t v, uint32_t identity, Op op, uint32_t* wtot) {
  uint32_t total;
  return msk_block_excl_scan<REV>(v, identity, op, wtot, &total);
}

// ---- wave-aggregated LDS histogram add -------------------------------------------------------------------------------------------
// A slot is one voxel per lane.  A label volume is mostly one class, so most slots hold one key 64 times, and 64 LDS atomics on one
// address serialise.  msk_count_slot peels keys off the slot: it takes the key of the first remaining lane, ballots the lanes
// that hold the same key and, when they are kMskPeelMin or more, adds their number with ONE single-lane LDS atomic.  Up to kMskPeel
// keys are peeled; after kMskPeelMiss keys that were held by fewer than kMskPeelMin lanes the slot counts as "scattered" (many
// classes, random data) and the remaining lanes add 1 each: such lanes share an address with at most a few others.
constexpr int kMskPeel = 8;        // most keys peeled off one slot
constexpr int kMskPeelMin = 4;     // a key held by fewer lanes is left to the per-lane adds (<= 3 adds on one address)
constexpr int kMskPeelMiss = 2;    // such keys in one slot before the peeling stops

// one voxel per lane, key < 0 = no voxel; called by every lane of the wavefront
__device__ __forceinline__ void msk_count_slot(int key, uint32_t* __restrict__ hist, int lane) {
  unsigned long long rest = __ballot(key >= 0);
  unsigned long long single = 0;
  int miss = 0;
  for (int it = 0; it < kMskPeel && rest != 0 && miss < kMskPeelMiss; ++it) {
    const int first = __ffsll((long long)rest) - 1;
    const int k = __builtin_amdgcn_readlane(key, first);
    const unsigned long long m = __ballot(key == k);   // a subset of rest: every lane of an earlier key has left it
    const int c = __popcll(m);
    if (c >= kMskPeelMin) {
      if (lane == first) atomicAdd(&hist[k], (uint32_t)c);
    } else {
      single |= m;
      ++miss;
    }
    rest &= ~m;
  }
  if (((rest | single) >> lane) & 1) atomicAdd(&hist[key], 1u);
}

// ---- the fixed-order float64 reduction ---------------------------------------------------------------------------------------------
// sum of squares of n floats (STATS: also sum, min and max) with an order of additions that is part of the result: the numpy
// statements reproduce it bit for bit.  Two passes:
//   chunk   one WAVEFRONT per chunk of kMskRedChunk = 4096 elements.  The statement's lane l of 256 adds x[l], x[l+256], ... in
//           float64; thread m of 64 carries the four lanes 4m .. 4m+3: its 16 loads are the quads 64j + m, j = 0..15, so every
//           load instruction of the wavefront is 1 KiB of consecutive bytes and all 16 are issued before the first add.  The tree
//           v[l] += v[l+s] is a xor butterfly over m for s = 128 .. 4 (a + b == b + a bit for bit) and two additions inside the
//           thread for s = 2, 1.  min / max ride along.  A pointer that is only 4-byte aligned and the last, partial chunk take
//           the same lanes one element at a time; elements past n add the statement's + 0.0 (it turns a -0.0 into +0.0).
//   finish  one workgroup of 256 over the chunk values P: lane l adds P[l], P[l+256], ... in ascending order, eight loads in
//           flight, then the LDS tree.
// The files that instantiate these compile with different contraction settings (msk_intensity.hip rounds every multiply and add
// on its own, msk_clip.hip does not).  Whichever setting reaches the bodies here, the bits are the same: (double)x * (double)x is
// exact (48 bits of product), so a fused multiply-add rounds as a multiply and an add do, and nothing else below multiplies.
constexpr int kMskRedChunk = 4096;   // elements per chunk
constexpr int kMskRedLanes = 256;    // lanes of the statement = threads of the finish pass

static inline long msk_chunks_of(size_t n) { return (long)((n + kMskRedChunk - 1) / kMskRedChunk); }

__device__ __forceinline__ double msk_shfl_xor_d(double v, int mask) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_xor(lo, mask, 64);
  hi = __shfl_xor(hi, mask, 64);
  return __hiloint2double(hi, lo);
}

struct msk_red_vals {   // without STATS only sumsq means anything
  double sum, sumsq;
  float mn, mx;
};

// called by the 64 threads of workgroup blockIdx.x = chunk; vec: x is 16-byte aligned.  The chunk's values, in every thread.
template <bool STATS>
__device__ __forceinline__ msk_red_vals msk_red_chunk(const float* __restrict__ x, long n, bool vec) {
  const int m = threadIdx.x;
  const long base = (long)blockIdx.x * kMskRedChunk;
  const long left = n - base;                       // >= 1
  double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
  float mn = INFINITY, mx = -INFINITY;
  if (vec && left >= kMskRedChunk) {
    const float4* x4 = reinterpret_cast<const float4*>(x + base);
    float4 v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = x4[64 * j + m];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double d = (double)e[i];
        if (STATS) s[i] = s[i] + d;
        q[i] = q[i] + d * d;
        if (STATS) mn = fminf(mn, e[i]);
        if (STATS) mx = fmaxf(mx, e[i]);
      }
    }
  } else {
    const float* xc = x + base;
    for (int j = 0; j < 16; ++j) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long e = 256L * j + 4 * m + i;
        if (e < left) {
          const float f = xc[e];
          const double d = (double)f;
          if (STATS) s[i] = s[i] + d;
          q[i] = q[i] + d * d;
          if (STATS) mn = fminf(mn, f);
          if (STATS) mx = fmaxf(mx, f);
        } else {                                    // the statement's + 0.0
          if (STATS) s[i] = s[i] + 0.0;
          q[i] = q[i] + 0.0;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                // s = 128 .. 4 of the tree
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (STATS) s[i] = s[i] + msk_shfl_xor_d(s[i], o);
      q[i] = q[i] + msk_shfl_xor_d(q[i], o);
    }
    if (STATS) mn = fminf(mn, __shfl_xor(mn, o, 64));
    if (STATS) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  msk_red_vals r;
  r.sum = (s[0] + s[2]) + (s[1] + s[3]);            // s = 2, then s = 1
  r.sumsq = (q[0] + q[2]) + (q[1] + q[3]);
  r.mn = mn;
  r.mx = mx;
  return r;
}

// called by the one workgroup of kMskRedLanes threads over the nc chunk values (psum, pmn, pmx: read with STATS only).  The
// values of the whole array, in every thread.
template <bool STATS>
__device__ __forceinline__ msk_red_vals msk_red_finish(long nc, const double* __restrict__ psum, const double* __restrict__ psq,
                                                       const float* __restrict__ pmn, const float* __restrict__ pmx) {
  constexpr int L = kMskRedLanes;
  __shared__ double ts[STATS ? L : 1], tq[L];
  __shared__ float tmn[STATS ? L : 1], tmx[STATS ? L : 1];
  const int l = threadIdx.x;
  double s = 0.0, q = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  long c = l;
  for (; c + 7L * L < nc; c += 8L * L) {            // eight loads in flight, added in order
    double a[8], b[8];
    float lo[8], hi[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      b[u] = psq[c + (long)u * L];
      if (STATS) {
        a[u] = psum[c + (long)u * L];
        lo[u] = pmn[c + (long)u * L];
        hi[u] = pmx[c + (long)u * L];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      q = q + b[u];
      if (STATS) {
        s = s + a[u];
        mn = fminf(mn, lo[u]);
        mx = fmaxf(mx, hi[u]);
      }
    }
  }
  for (; c < nc; c += L) {
    q = q + psq[c];
    if (STATS) {
      s = s + psum[c];
      mn = fminf(mn, pmn[c]);
      mx = fmaxf(mx, pmx[c]);
    }
  }
  tq[l] = q;
  if (STATS) { ts[l] = s; tmn[l] = mn; tmx[l] = mx; }
  __syncthreads();
  for (int o = L / 2; o > 0; o >>= 1) {
    if (l < o) {
      tq[l] = tq[l] + tq[l + o];
      if (STATS) {
        ts[l] = ts[l] + ts[l + o];
        tmn[l] = fminf(tmn[l], tmn[l + o]);
        tmx[l] = fmaxf(tmx[l], tmx[l + o]);
      }
    }
    __syncthreads();
  }
  msk_red_vals r;
  r.sumsq = tq[0];
  r.sum = STATS ? ts[0] : 0.0;
  r.mn = STATS ? tmn[0] : 0.f;
  r.mx = STATS ? tmx[0] : 0.f;
  return r;
}

// ---- the radix select's keys, histograms and digit resolution ----------------------------------------------------------------------
// What msk_loss_topk.hip (the K-th largest loss) and msk_normalize.hip (two order statistics of the valid voxels) share; the
// statements are tests/topk_reference.py and tests/normalize_reference.py.  Values are ordered by the sortable key of their bit
// pattern (sign set: all bits flipped, else the sign bit set: -0.0 < +0.0, nothing is left to a float comparison).  Three digits
// of 11, 11 and 10 bits, most significant first; a workgroup of 256 threads counts a digit in an LDS histogram of 2048 bins and
// merges it into a global one with integer atomics, and every later pass rescans the global histograms in its prologue.
constexpr int kMskSelThreads = 256;
constexpr int kMskSelPasses = 3;     // digits of 11, 11 and 10 bits, most significant first
constexpr int kMskSelBins = 2048;    // bins per digit: eight consecutive bins per thread of the workgroup that rescans a histogram
constexpr int kMskSelBinsPerThread = kMskSelBins / kMskSelThreads;
__host__ __device__ constexpr int msk_sel_shift(int p) { return p == 0 ? 21 : (p == 1 ? 10 : 0); }
__host__ __device__ constexpr int msk_sel_width(int p) { return p == 2 ? 10 : 11; }

__device__ __forceinline__ uint32_t msk_sel_key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float msk_sel_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

struct msk_sel {
  uint32_t K;        // 0: nothing is selected, the other fields mean nothing
  uint32_t prefix;   // the digits of the K-th largest key found so far
  uint32_t krem;     // the rank sought among the keys that carry them
  uint32_t ngt;      // keys above every key that carries them
  uint32_t neq;      // keys that carry them
};

// a thread's eight consecutive bins of the global histograms of passes 0 .. NP-1 (16-byte aligned): asked for at once, one round trip
template <int NP>
struct msk_sel_bins {
  uint4 lo[NP], hi[NP];
};
template <int NP>
__device__ __forceinline__ msk_sel_bins<NP> msk_sel_load(const uint32_t* const* hist) {
  msk_sel_bins<NP> b;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const uint4* h = reinterpret_cast<const uint4*>(hist[p]) + 2 * threadIdx.x;
    b.lo[p] = h[0];
    b.hi[p] = h[1];
  }
  return b;
}

// The first NP digits of the K-th largest key from the bins msk_sel_load returned; K <= the number of keys.  Called by all 256
// threads; s_scan: 8 LDS words.  Per digit a thread holds eight consecutive bins: the exclusive scan over the threads ABOVE
// it, then the one thread with above < krem <= above + count walks its bins down from the top.  K == 0 returns before any
// barrier (K must be uniform over the workgroup).
template <int NP>
__device__ __forceinline__ msk_sel msk_sel_scan(const msk_sel_bins<NP>& b, uint32_t K, uint32_t* s_scan) {
  msk_sel s = {K, 0u, K, 0u, 0u};
  if (K == 0) return s;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const uint32_t c8[kMskSelBinsPerThread] = {b.lo[p].x, b.lo[p].y, b.lo[p].z, b.lo[p].w, b.hi[p].x, b.hi[p].y, b.hi[p].z, b.hi[p].w};
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kMskSelBinsPerThread; ++j) c += c8[j];
    uint32_t above = msk_block_excl_scan<true>(c, 0u, msk_op_add(), s_scan);
    if (s.krem > above && s.krem - above <= c) {
      int j = kMskSelBinsPerThread - 1;
      for (; j > 0 && s.krem - above > c8[j]; --j) above += c8[j];
      s_scan[4] = kMskSelBinsPerThread * threadIdx.x + j;
      s_scan[5] = above;
      s_scan[6] = c8[j];
    }
    __syncthreads();   // (the next digit writes these words behind the two barriers of its scan)
    s.prefix = (s.prefix << msk_sel_width(p)) | s_scan[4];
    s.ngt += s_scan[5];
    s.krem -= s_scan[5];
    s.neq = s_scan[6];
  }
  return s;
}

// the workgroup's LDS histogram: cleared (a barrier must follow) and added to the global one (behind a barrier); empty bins cost
// no atomic (adding them too, so that a wavefront's atomics cover consecutive words, was measured 4 us per pass slower)
__device__ __forceinline__ void msk_sel_hist_clear(uint32_t* __restrict__ s_hist) {
  for (int b = threadIdx.x; b < kMskSelBins; b += kMskSelThreads) s_hist[b] = 0u;
}
__device__ __forceinline__ void msk_sel_hist_merge(const uint32_t* __restrict__ s_hist, uint32_t* __restrict__ g_hist) {
  for (int b = threadIdx.x; b < kMskSelBins; b += kMskSelThreads) {
    const uint32_t c = s_hist[b];
    if (c) atomicAdd(&g_hist[b], c);
  }
}

// the tree of msk_red_chunk over the four lane values a thread of the chunk's wavefront carries
__device__ __forceinline__ double msk_red_chunk_tree(double (&s)[4]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                     // s = 128 .. 4 of the tree
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = s[i] + msk_shfl_xor_d(s[i], o);
  }
  return (s[0] + s[2]) + (s[1] + s[3]);                  // s = 2, then s = 1
}
