// Intensity augmentation of a float32 volume that lives on the device (transforms.RandomGaussianNoise3D, RandomGaussianBlur3D,
// RandomBrightness3D, RandomContrast3D, RandomGamma3D; tests/intensity_reference.py is the statement): statistics, one
// streaming elementwise pass, and a separable Gaussian blur.  Nothing here synchronises, downloads or uses an atomic; the
// statistics a transform needs are read from a DEVICE record by the pass that uses them, so a whole transform is enqueued
// without the host ever seeing a value.
//
//   stats   the fixed-order float64 reduction of msk_device.h (msk_red_chunk / msk_red_finish, the one msk_grad_clip_coef uses)
//           with sum, min and max riding along: one wavefront per chunk of 4096 voxels, the chunk values go to the workspace
//           (24 bytes per 16 KiB of volume), and a second launch of one workgroup reduces them.
//   apply   a workgroup takes tiles of 1024 quads (four 16-byte loads per lane, issued together) in a grid-stride loop, so
//           the scalars derived from the records (a float64 division, a square root) are computed once per thread and not
//           once per quad; a scalar form for pointers that are only 4-byte aligned and for the last n % 4 elements.
//   blur    up to three passes.  Along D and H a thread owns one column of kSeg = 16 consecutive outputs of the filtered axis:
//           it loads 16 + 2r values (lanes = consecutive addresses of the contiguous axis), keeps them in registers and
//           writes 16 results, so the pass reads (16 + 2r) / 16 of the volume whatever the caches hold.  Along W a workgroup
//           stages 1024 consecutive voxels of the FLATTENED volume plus 8 on either side in LDS: reflect() never moves a
//           neighbour further than r <= 8 from its voxel and never out of its row, so every operand is in the tile, for any
//           W (rows shorter than the workgroup included) and with every lane busy.
#include "msk_common.h"

#pragma clang fp contract(off)   // for the whole file: every multiply and add below is rounded on its own

namespace {

constexpr int kMaxR = 8;         // blur radius
constexpr int kSeg = 16;         // outputs per thread of the column passes
constexpr int kTile = 1024;      // outputs per workgroup of the W pass
constexpr int kThreads = 256;

// ---- statistics --------------------------------------------------------------------------------------------------------------
// workspace: sum[nc], sumsq[nc] (double), mn[nc], mx[nc] (float)
// grid: one wavefront (64 threads) per chunk
__global__ void __launch_bounds__(64)
intensity_chunk_k(const float* __restrict__ x, long n, int vec, long nc, double* __restrict__ psum, double* __restrict__ psq,
                  float* __restrict__ pmn, float* __restrict__ pmx) {
  const msk_red_vals r = msk_red_chunk<true>(x, n, vec != 0);
  if (threadIdx.x == 0) {
    psum[blockIdx.x] = r.sum;
    psq[blockIdx.x] = r.sumsq;
    pmn[blockIdx.x] = r.mn;
    pmx[blockIdx.x] = r.mx;
  }
}

// one workgroup of 256; thread 0 writes the record
__global__ void __launch_bounds__(kMskRedLanes)
intensity_finish_k(long nc, const double* __restrict__ psum, const double* __restrict__ psq, const float* __restrict__ pmn,
                   const float* __restrict__ pmx, double* __restrict__ stats) {
  const msk_red_vals r = msk_red_finish<true>(nc, psum, psq, pmn, pmx);
  if (threadIdx.x == 0) {
    stats[0] = (double)r.mn;
    stats[1] = (double)r.mx;
    stats[2] = r.sum;
    stats[3] = r.sumsq;
  }
}

// ---- the elementwise pass ----------------------------------------------------------------------------------------------------
struct ApplyArgs {
  float p[4];
  long n;
  uint64_t key;    // splitmix64(seed)
};

template <int MODE>
struct ApplyOp {
  float a = 0.f, b = 0.f, c = 0.f, d = 0.f, sgn = 1.f;
  bool clamp = false;
  uint64_t key = 0;

  __device__ __forceinline__ ApplyOp(const ApplyArgs& g, const double* __restrict__ sa, const double* __restrict__ sb) {
    if (MODE == MSK_INTENSITY_NOISE) {
      a = g.p[0];
      key = g.key;
    } else if (MODE == MSK_INTENSITY_SCALE) {
      a = g.p[0];
    } else if (MODE == MSK_INTENSITY_CONTRAST) {
      a = g.p[0];
      b = (float)(sa[2] / (double)g.n);            // the mean
      clamp = g.p[1] != 0.f;
      c = (float)sa[0];
      d = (float)sa[1];
    } else if (MODE == MSK_INTENSITY_GAMMA) {
      a = g.p[0];
      const bool inv = g.p[1] != 0.f;
      sgn = inv ? -1.f : 1.f;
      const float mn = inv ? -(float)sa[1] : (float)sa[0], mx = inv ? -(float)sa[0] : (float)sa[1];
      b = mn;
      c = mx - mn;                                 // rg
      d = c + 1e-7f;
    } else {
      const double n = (double)g.n;
      const double ma = sa[2] / n, mb = sb[2] / n;
      double va = sa[3] / n - ma * ma, vb = sb[3] / n - mb * mb;
      va = va > 0.0 ? va : 0.0;
      vb = vb > 0.0 ? vb : 0.0;
      a = (float)ma;                               // mean_A
      b = (float)sqrt(va);                         // sd_A
      c = (float)mb;                               // mean_B
      d = (float)sqrt(vb) + 1e-8f;                 // sd_B + 1e-8
    }
  }

  __device__ __forceinline__ float operator()(float x, long i) const {
    if (MODE == MSK_INTENSITY_NOISE) {
      const uint64_t h = splitmix64(key + (uint64_t)i);
      const float u1 = (float)((uint32_t)(h >> 40) + 1u) * (1.0f / 16777216.0f);
      const float u2 = (float)((uint32_t)(h >> 8) & 0xFFFFFFu) * (1.0f / 16777216.0f);
      const float z = sqrtf(-2.0f * logf(u1)) * cosf(6.2831853071795864769f * u2);
      return x + a * z;
    } else if (MODE == MSK_INTENSITY_SCALE) {
      return x * a;
    } else if (MODE == MSK_INTENSITY_CONTRAST) {
      float y = ((x - b) * a) + b;
      if (clamp) y = fminf(fmaxf(y, c), d);
      return y;
    } else if (MODE == MSK_INTENSITY_GAMMA) {
      const float t = (sgn * x - b) / d;
      return sgn * (powf(t, a) * c + b);
    } else {
      return (x - c) / d * b + a;
    }
  }
};

// tiles of 1024 quads per workgroup, grid-stride; then the n % 4 tail (first workgroup)
template <int MODE>
__global__ void __launch_bounds__(kThreads)
intensity_apply_vec_k(const float* __restrict__ x, float* __restrict__ y, const ApplyArgs g, const double* __restrict__ sa,
                      const double* __restrict__ sb) {
  const ApplyOp<MODE> op(g, sa, sb);
  const long nq = g.n >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float4* y4 = reinterpret_cast<float4*>(y);
  for (long t0 = (long)blockIdx.x * 1024; t0 < nq; t0 += (long)gridDim.x * 1024) {
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long qi = t0 + k * kThreads + threadIdx.x;
      if (qi < nq) v[k] = x4[qi];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long qi = t0 + k * kThreads + threadIdx.x;
      if (qi < nq) {
        float4 r;
        r.x = op(v[k].x, 4 * qi);
        r.y = op(v[k].y, 4 * qi + 1);
        r.z = op(v[k].z, 4 * qi + 2);
        r.w = op(v[k].w, 4 * qi + 3);
        y4[qi] = r;
      }
    }
  }
  if (blockIdx.x == 0) {
    const long i = 4 * nq + threadIdx.x;
    if (threadIdx.x < 4 && i < g.n) y[i] = op(x[i], i);
  }
}

template <int MODE>
__global__ void __launch_bounds__(kThreads)
intensity_apply_elem_k(const float* __restrict__ x, float* __restrict__ y, const ApplyArgs g, const double* __restrict__ sa,
                       const double* __restrict__ sb) {
  const ApplyOp<MODE> op(g, sa, sb);
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < g.n; i += (long)gridDim.x * kThreads) y[i] = op(x[i], i);
}

template <int MODE>
void launch_apply(msk_ctx* ctx, const float* x, float* y, const ApplyArgs& g, const double* sa, const double* sb) {
  const bool vec = ((((uintptr_t)x) | ((uintptr_t)y)) & 15) == 0 && g.n >= 4;
  const long cap = (long)ctx->num_cu * 8;
  if (vec) {
    const long tiles = ((g.n >> 2) + 1023) / 1024;
    hipLaunchKernelGGL(intensity_apply_vec_k<MODE>, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(kThreads), 0, ctx->stream, x, y, g,
                       sa, sb);
  } else {
    const long blocks = (g.n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(intensity_apply_elem_k<MODE>, dim3((unsigned)(blocks < 4 * cap ? blocks : 4 * cap)), dim3(kThreads), 0,
                       ctx->stream, x, y, g, sa, sb);
  }
}

// ---- blur --------------------------------------------------------------------------------------------------------------------
struct Taps {
  float w[2 * kMaxR + 1];
};

// scipy's 'reflect' (d c b a | a b c d | d c b a) for any i and any extent n >= 1: mirror about -1/2 and n - 1/2 until inside
// (|i| shrinks by n per turn; the callers are at most 8 outside, so at most 9 turns), which equals m < n ? m : 2n-1-m, m = i mod 2n
__device__ __forceinline__ int reflect_idx(int i, int n) {
  while ((unsigned)i >= (unsigned)n) i = i < 0 ? -i - 1 : n - 1 - (i - n);
  return i;
}

// the volume as [outer][L][inner], filtered along L.  thread: one (outer, inner) column, kSeg outputs from blockIdx.y * kSeg.
// Offsets are 32-bit: the volume has fewer than 2^31 voxels.
template <int R>
__global__ void __launch_bounds__(kThreads)
blur_column_k(const float* __restrict__ src, float* __restrict__ dst, int columns, int L, int inner, const Taps taps) {
  const int col = blockIdx.x * kThreads + threadIdx.x;
  if (col >= columns) return;
  const int o = col / inner, c = col - o * inner;
  const int base = o * L * inner + c;
  const int i0 = blockIdx.y * kSeg;                  // the same in every thread, like everything that follows from it
  const int cnt = L - i0 < kSeg ? L - i0 : kSeg;      // >= 1
  float v[kSeg + 2 * R];
  if (i0 >= R && i0 + kSeg + R <= L) {                // no operand is mirrored
    const float* q = src + base + (i0 - R) * inner;
#pragma unroll
    for (int j = 0; j < kSeg + 2 * R; ++j) v[j] = q[j * inner];
  } else {                                            // every index is mirrored into the column, also those no output needs
#pragma unroll
    for (int j = 0; j < kSeg + 2 * R; ++j) v[j] = src[base + reflect_idx(i0 - R + j, L) * inner];
  }
  float* out = dst + base + i0 * inner;
#pragma unroll
  for (int i = 0; i < kSeg; ++i) {
    float acc = taps.w[0] * v[i];
#pragma unroll
    for (int k = 1; k <= 2 * R; ++k) acc = acc + taps.w[k] * v[i + k];
    if (i < cnt) out[i * inner] = acc;
  }
}

// filtered along the contiguous axis: kTile consecutive voxels of the flattened volume per workgroup
template <int R>
__global__ void __launch_bounds__(kThreads)
blur_row_k(const float* __restrict__ src, float* __restrict__ dst, long n, int W, const Taps taps) {
  __shared__ float tile[kTile + 2 * kMaxR];
  const long g0 = (long)blockIdx.x * kTile;
  const int t = threadIdx.x;
  for (int j = t; j < kTile + 2 * kMaxR; j += kThreads) {
    const long g = g0 - kMaxR + j;
    tile[j] = (g >= 0 && g < n) ? src[g] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kTile / kThreads; ++u) {
    const int j = u * kThreads + t;
    const long g = g0 + j;
    if (g >= n) break;
    const int col = (int)((unsigned)g % (unsigned)W);   // n < 2^31
    const float* p = tile + kMaxR + j - col;            // p[c] = the row's column c (for the columns inside the tile)
    float acc = taps.w[0] * p[reflect_idx(col - R, W)];
#pragma unroll
    for (int k = 1; k <= 2 * R; ++k) acc = acc + taps.w[k] * p[reflect_idx(col - R + k, W)];
    dst[g] = acc;
  }
}

template <int R>
void launch_column(msk_ctx* ctx, const float* src, float* dst, long outer, int L, long inner, const Taps& taps) {
  const int columns = (int)(outer * inner);
  hipLaunchKernelGGL(blur_column_k<R>, dim3((unsigned)((columns + kThreads - 1) / kThreads), (unsigned)((L + kSeg - 1) / kSeg)),
                     dim3(kThreads), 0, ctx->stream, src, dst, columns, L, (int)inner, taps);
}
template <int R>
void launch_row(msk_ctx* ctx, const float* src, float* dst, long n, int W, const Taps& taps) {
  hipLaunchKernelGGL(blur_row_k<R>, dim3((unsigned)((n + kTile - 1) / kTile)), dim3(kThreads), 0, ctx->stream, src, dst, n, W, taps);
}

#define MSK_BLUR_DISPATCH(r, fn, ...)      \
  switch (r) {                             \
    case 1: fn<1>(__VA_ARGS__); break;     \
    case 2: fn<2>(__VA_ARGS__); break;     \
    case 3: fn<3>(__VA_ARGS__); break;     \
    case 4: fn<4>(__VA_ARGS__); break;     \
    case 5: fn<5>(__VA_ARGS__); break;     \
    case 6: fn<6>(__VA_ARGS__); break;     \
    case 7: fn<7>(__VA_ARGS__); break;     \
    default: fn<8>(__VA_ARGS__); break;    \
  }

}  // namespace

extern "C" {

int msk_intensity_stats_workspace(long n, size_t* bytes) {
  MSK_REQUIRE(nullptr, bytes != nullptr, "bytes must not be null");
  MSK_REQUIRE(nullptr, n >= 1 && n <= 0x7fffffffL, "n must be in [1, 2^31)");
  *bytes = ((size_t)msk_chunks_of((size_t)n) * 24 + 255) & ~(size_t)255;
  return 0;
}

int msk_intensity_stats(msk_ctx* ctx, const float* x, long n, void* workspace, double* stats) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, x != nullptr && workspace != nullptr && stats != nullptr, "null x / workspace / stats");
  MSK_REQUIRE(ctx, n >= 1 && n <= 0x7fffffffL, "n must be in [1, 2^31)");
  MSK_REQUIRE(ctx, (((uintptr_t)x) & 3) == 0, "x must be 4-byte aligned");
  MSK_REQUIRE(ctx, ((((uintptr_t)workspace) | ((uintptr_t)stats)) & 7) == 0, "workspace / stats must be 8-byte aligned");
  const long nc = msk_chunks_of((size_t)n);
  double* psum = (double*)workspace;
  double* psq = psum + nc;
  float* pmn = (float*)(psq + nc);
  float* pmx = pmn + nc;
  const int vec = (((uintptr_t)x) & 15) == 0;
  {
    msk_launch_scope ls(ctx, "intensity_stats");
    hipLaunchKernelGGL(intensity_chunk_k, dim3((unsigned)nc), dim3(64), 0, ctx->stream, x, n, vec, nc, psum, psq, pmn, pmx);
  }
  {
    msk_launch_scope ls(ctx, "intensity_stats_finish");
    hipLaunchKernelGGL(intensity_finish_k, dim3(1), dim3(kMskRedLanes), 0, ctx->stream, nc, (const double*)psum, (const double*)psq,
                       (const float*)pmn, (const float*)pmx, stats);
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

int msk_intensity_apply(msk_ctx* ctx, const float* x, float* y, long n, int mode, const float* params, const double* stats_a,
                        const double* stats_b, uint64_t seed) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, x != nullptr && y != nullptr && params != nullptr, "null x / y / params");
  MSK_REQUIRE(ctx, n >= 1 && n <= 0x7fffffffL, "n must be in [1, 2^31)");
  MSK_REQUIRE(ctx, ((((uintptr_t)x) | ((uintptr_t)y)) & 3) == 0, "x / y must be 4-byte aligned");
  MSK_REQUIRE(ctx, ((((uintptr_t)stats_a) | ((uintptr_t)stats_b)) & 7) == 0, "stats records must be 8-byte aligned");
  MSK_REQUIRE(ctx, mode >= MSK_INTENSITY_NOISE && mode <= MSK_INTENSITY_RESTORE, "mode must be one of MSK_INTENSITY_*");
  MSK_REQUIRE(ctx, mode < MSK_INTENSITY_CONTRAST || stats_a != nullptr, "this mode needs stats_a");
  MSK_REQUIRE(ctx, mode != MSK_INTENSITY_RESTORE || stats_b != nullptr, "RESTORE needs stats_b");
  MSK_REQUIRE(ctx, (const float*)y == x || msk_bytes_disjoint(x, (size_t)n * 4, y, (size_t)n * 4), "y must be x or not overlap it");
  ApplyArgs g;
  for (int i = 0; i < 4; ++i) g.p[i] = params[i];
  g.n = n;
  g.key = splitmix64(seed);
  msk_launch_scope ls(ctx, "intensity_apply");
  switch (mode) {
    case MSK_INTENSITY_NOISE: launch_apply<MSK_INTENSITY_NOISE>(ctx, x, y, g, stats_a, stats_b); break;
    case MSK_INTENSITY_SCALE: launch_apply<MSK_INTENSITY_SCALE>(ctx, x, y, g, stats_a, stats_b); break;
    case MSK_INTENSITY_CONTRAST: launch_apply<MSK_INTENSITY_CONTRAST>(ctx, x, y, g, stats_a, stats_b); break;
    case MSK_INTENSITY_GAMMA: launch_apply<MSK_INTENSITY_GAMMA>(ctx, x, y, g, stats_a, stats_b); break;
    default: launch_apply<MSK_INTENSITY_RESTORE>(ctx, x, y, g, stats_a, stats_b); break;
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

int msk_gauss_blur3d(msk_ctx* ctx, const float* x, float* y, int d, int h, int w, const float* taps_d, int r_d, const float* taps_h,
                     int r_h, const float* taps_w, int r_w, float* tmp) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, x != nullptr && y != nullptr, "null x / y");
  MSK_REQUIRE(ctx, d >= 1 && h >= 1 && w >= 1, "extents must be >= 1");
  MSK_REQUIRE(ctx, (long)d * h * w <= 0x7fffffffL, "the volume must have fewer than 2^31 voxels");
  MSK_REQUIRE(ctx, r_d >= 0 && r_d <= kMaxR && r_h >= 0 && r_h <= kMaxR && r_w >= 0 && r_w <= kMaxR, "radii must be in [0, 8]");
  MSK_REQUIRE(ctx, (r_d == 0 || taps_d != nullptr) && (r_h == 0 || taps_h != nullptr) && (r_w == 0 || taps_w != nullptr),
              "taps must be host arrays of 2r+1 floats");
  MSK_REQUIRE(ctx, ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)tmp)) & 3) == 0, "x / y / tmp must be 4-byte aligned");
  const long n = (long)d * h * w;
  const size_t bytes = (size_t)n * 4;
  MSK_REQUIRE(ctx, msk_bytes_disjoint(x, bytes, y, bytes), "y must not overlap x");
  const int passes = (r_d > 0) + (r_h > 0) + (r_w > 0);
  if (passes >= 2) {
    MSK_REQUIRE(ctx, tmp != nullptr, "two or three blurred axes need tmp");
    MSK_REQUIRE(ctx, msk_bytes_disjoint(tmp, bytes, x, bytes) && msk_bytes_disjoint(tmp, bytes, y, bytes), "tmp must overlap neither x nor y");
  }
  if (passes == 0) {
    MSK_CHECK_HIP(ctx, hipMemcpyAsync(y, x, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
  }
  msk_launch_scope ls(ctx, "gauss_blur3d");
  // the chain ends in y: x -> y;  x -> tmp -> y;  x -> y -> tmp -> y
  const float* src = x;
  int left = passes;
  const int rs[3] = {r_d, r_h, r_w};
  const float* ts[3] = {taps_d, taps_h, taps_w};
  for (int axis = 0; axis < 3; ++axis) {
    const int r = rs[axis];
    if (r == 0) continue;
    float* dst = (left % 2 == 1) ? y : tmp;
    Taps taps;
    memset(&taps, 0, sizeof(taps));
    for (int k = 0; k < 2 * r + 1; ++k) taps.w[k] = ts[axis][k];
    if (axis == 0) {
      MSK_BLUR_DISPATCH(r, launch_column, ctx, src, dst, 1L, d, (long)h * w, taps)
    } else if (axis == 1) {
      MSK_BLUR_DISPATCH(r, launch_column, ctx, src, dst, (long)d, h, (long)w, taps)
    } else {
      MSK_BLUR_DISPATCH(r, launch_row, ctx, src, dst, n, w, taps)
    }
    src = dst;
    --left;
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
