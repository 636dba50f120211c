// Exact squared Euclidean distance transform of an int32 label volume [D, H, W] (axes z, y, x) and the surface-voxel
// gather on top of it: the device half of utils.metric.edt_squared / surface_distances (Hausdorff, HD95, ASSD).
//
// Specification (utils/metric.py states it in numpy; the kernels return exactly these bits):
//   features F = {vol == cls}, or its surface S = the voxels of F with a face neighbour outside F (beyond the volume's
//   edge counts as outside), or -- msk_edt_field with `complement`, for the signed distance maps of msk_loss_boundary.hip --
//   the complement {vol != cls};  wx, wy, wz = the squared spacings, rounded once;
//   dist2(v) = min over u in F of fl(fl(fl(wx dx^2) + fl(wy dy^2)) + fl(wz dz^2)),  +inf when F is empty,
// every fl one float64 rounding, no fused multiply-add (contraction is switched off for this file and the kernels'
// code objects hold no v_fma_f64).  Rounding is monotone, so the minimum separates:
//   x pass  gx(x)  = wx * dx^2 of the nearest feature of the row (one rounding; dx^2 is an exact integer);
//   y pass  gy(y)  = min over y' of fl(gx(y') + fl(wy (y - y')^2));
//   z pass  the same along z on gy.
//
// x pass (edt_x_k): one wavefront per row.  The feature flags of a row become W / 64 ballot words in LDS; a lane finds
// the nearest set bit on either side of its voxel with clz / ffs on those words.  Reads 4 bytes (the volume; the
// surface test's neighbours come from L2), writes 8 bytes per voxel, both contiguous along x.
//
// y and z pass (edt_line_k): a workgroup owns ALL entries of 2^tx_shift neighbouring lines (neighbouring in x, so that
// every global access is a run of 8 * 2^tx_shift contiguous bytes) in an LDS tile [L][TX] of at most kTileBytes (plus TX
// int flags, one per line); it loads the tile, then thread (l, tx) takes the minimum over the line by brute force from LDS, stepping outwards
// (l - k, l + k for k = 1, 2, ...) and stopping once w k^2 alone is >= the running best: every later candidate is
// fl(g + fl(w k^2)) >= fl(w k^2) >= best.  Exact by construction (no intersection points, no division); the work per
// voxel is proportional to its distance from the nearest feature along the line, and neighbouring lanes stop at
// nearly the same k.  Lines without a finite entry are skipped (their result is the +inf they already hold).  The
// pass runs in place: a workgroup reads its whole tile before it writes, and tiles are disjoint.  No workgroup waits
// for another: the three passes are three launches.
//
// Extents: 1 .. MSK_EDT_MAX_EXTENT (2048) per axis: a line of 2048 doubles with TX = 2 fills the 32 KiB tile (+ 8 bytes of flags).
#include "msk_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxExtent = MSK_EDT_MAX_EXTENT;
constexpr int kMaxWords = kMaxExtent / 64;
constexpr int kTileBytes = 32768;

struct Vol {
  const int32_t* p;
  int d, h, w, cls, surface;
  int complement;   // the features are {vol != cls} (msk_edt_field for msk_label_sdf; never with surface)
};

// is voxel (z, y, x), whose value is v, a feature?
__device__ __forceinline__ bool edt_feature(const Vol& g, long i, int z, int y, int x, int v) {
  if (g.complement) return v != g.cls;
  if (v != g.cls) return false;
  if (!g.surface) return true;
  if (x == 0 || x == g.w - 1 || y == 0 || y == g.h - 1 || z == 0 || z == g.d - 1) return true;
  const long sy = g.w, sz = (long)g.h * g.w;
  return g.p[i - 1] != g.cls || g.p[i + 1] != g.cls || g.p[i - sy] != g.cls || g.p[i + sy] != g.cls ||
         g.p[i - sz] != g.cls || g.p[i + sz] != g.cls;
}

// grid: rows / kWaves workgroups at most; every wavefront of a workgroup makes the same number of trips
__global__ void __launch_bounds__(kThreads)
edt_x_k(Vol g, double wx, double* __restrict__ out) {
  __shared__ unsigned long long words[kWaves][kMaxWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long rows = (long)g.d * g.h;
  const int nwords = (g.w + 63) >> 6;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  for (long row0 = (long)blockIdx.x * kWaves; row0 < rows; row0 += (long)gridDim.x * kWaves) {
    const long row = row0 + wave;
    const bool live = row < rows;
    const int z = live ? (int)(row / g.h) : 0, y = live ? (int)(row - (long)z * g.h) : 0;
    const long base = row * g.w;
    unsigned long long any = 0;
    for (int k = 0; k < nwords; ++k) {
      const int x = k * 64 + lane;
      bool f = false;
      if (live && x < g.w) f = edt_feature(g, base + x, z, y, x, g.p[base + x]);
      const unsigned long long m = __ballot(f);
      if (lane == 0) words[wave][k] = m;
      any |= m;
    }
    __syncthreads();
    if (live) {
      for (int x = lane; x < g.w; x += 64) {
        double r = inf;
        if (any) {
          const int wi = x >> 6, b = x & 63;
          int dl = -1, dr = -1;   // distance to the nearest feature at or left of x / right of x
          unsigned long long m = words[wave][wi] & (~0ULL >> (63 - b));
          for (int k = wi;;) {
            if (m) { dl = x - (k * 64 + 63 - __clzll((long long)m)); break; }
            if (--k < 0) break;
            m = words[wave][k];
          }
          m = words[wave][wi] & (~0ULL << b);
          for (int k = wi;;) {
            if (m) { dr = k * 64 + __ffsll((long long)m) - 1 - x; break; }
            if (++k >= nwords) break;
            m = words[wave][k];
          }
          const int dx = dl < 0 ? dr : (dr < 0 ? dl : (dl < dr ? dl : dr));
          r = wx * (double)(dx * dx);
        }
        out[base + x] = r;
      }
    }
    __syncthreads();
  }
}

// One pass along an axis of L entries `lstride` doubles apart; grid (tiles of TX = 1 << tx_shift lines along x, outer):
// the lines of one workgroup start at outer * ostride + x0 .. x0 + TX - 1.  Dynamic LDS: L * TX doubles + TX ints.
__global__ void __launch_bounds__(kThreads)
edt_line_k(double* __restrict__ g, int L, long lstride, long ostride, int W, int tx_shift, double w) {
  extern __shared__ double tile[];
  const int TX = 1 << tx_shift;
  int* colany = reinterpret_cast<int*>(tile + (size_t)L * TX);
  const int t = threadIdx.x;
  const int x0 = blockIdx.x << tx_shift;
  double* base = g + (long)blockIdx.y * ostride + x0;
  const int n = L << tx_shift;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  if (t < TX) colany[t] = 0;
  __syncthreads();
  for (int i = t; i < n; i += kThreads) {
    const int l = i >> tx_shift, tx = i & (TX - 1);
    double v = inf;
    if (x0 + tx < W) v = base[(long)l * lstride + tx];
    tile[i] = v;
    if (v < inf) colany[tx] = 1;   // every writer stores the same value
  }
  __syncthreads();
  for (int i = t; i < n; i += kThreads) {
    const int l = i >> tx_shift, tx = i & (TX - 1);
    if (!colany[tx]) continue;   // no feature on this line (or beyond W): the +inf stays
    double best = tile[i];
    const double first = best;
    double fk = 1.0;
    for (int k = 1;; ++k, fk += 1.0) {
      const bool lo = l - k >= 0, hi = l + k < L;
      if (!lo && !hi) break;
      const double c = w * (fk * fk);   // fk * fk is an exact integer
      if (c >= best) break;
      if (lo) {
        const double v = tile[i - (k << tx_shift)] + c;
        best = v < best ? v : best;
      }
      if (hi) {
        const double v = tile[i + (k << tx_shift)] + c;
        best = v < best ? v : best;
      }
    }
    if (best != first) base[(long)l * lstride + tx] = best;
  }
}

// grid-stride over the voxels; *count += surface voxels of {vol == cls}
__global__ void __launch_bounds__(kThreads)
surface_count_k(Vol g, unsigned long long* __restrict__ count) {
  __shared__ unsigned int part[kWaves];
  const long V = (long)g.d * g.h * g.w, sy = g.w, sz = (long)g.h * g.w;
  unsigned int mine = 0;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < V; i += (long)gridDim.x * kThreads) {
    const int v = g.p[i];
    if (v != g.cls) continue;
    const int z = (int)(i / sz);
    const long r = i - (long)z * sz;
    const int y = (int)(r / sy), x = (int)(r - (long)y * sy);
    mine += edt_feature(g, i, z, y, x, v) ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int s = 0;
    for (int k = 0; k < kWaves; ++k) s += part[k];
    if (s) atomicAdd(count, (unsigned long long)s);
  }
}

// out[slot] = dist2[v] for every surface voxel v, slots handed out by *count (one atomic per workgroup and trip);
// nothing is written at a slot >= capacity.  Every thread of a workgroup makes the same number of trips.
__global__ void __launch_bounds__(kThreads)
surface_gather_k(Vol g, const double* __restrict__ dist2, double* __restrict__ out, long capacity,
                 unsigned long long* __restrict__ count) {
  __shared__ unsigned int part[kWaves];
  __shared__ unsigned long long slot0;
  const long V = (long)g.d * g.h * g.w, sy = g.w, sz = (long)g.h * g.w;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long i0 = (long)blockIdx.x * kThreads; i0 < V; i0 += (long)gridDim.x * kThreads) {
    const long i = i0 + threadIdx.x;
    bool s = false;
    if (i < V) {
      const int v = g.p[i];
      if (v == g.cls) {
        const int z = (int)(i / sz);
        const long r = i - (long)z * sz;
        const int y = (int)(r / sy), x = (int)(r - (long)y * sy);
        s = edt_feature(g, i, z, y, x, v);
      }
    }
    const unsigned long long m = __ballot(s);
    if (lane == 0) part[wave] = (unsigned int)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned int tot = 0;
      for (int k = 0; k < kWaves; ++k) tot += part[k];
      slot0 = tot ? atomicAdd(count, (unsigned long long)tot) : 0ULL;
    }
    __syncthreads();
    if (s) {
      unsigned long long slot = slot0 + (unsigned long long)__popcll(m & ((1ULL << lane) - 1));
      for (int k = 0; k < wave; ++k) slot += part[k];
      if (slot < (unsigned long long)capacity) out[slot] = dist2[i];
    }
    __syncthreads();   // part / slot0 are rewritten by the next trip
  }
}

int check_volume(msk_ctx* ctx, const int32_t* vol, int d, int h, int w) {
  MSK_REQUIRE(ctx, vol != nullptr && (((uintptr_t)vol) & 3) == 0, "vol must be a 4-byte aligned device pointer");
  MSK_REQUIRE(ctx, d >= 1 && h >= 1 && w >= 1 && d <= kMaxExtent && h <= kMaxExtent && w <= kMaxExtent,
              "every extent must be in [1, 2048] (MSK_EDT_MAX_EXTENT)");
  return 0;
}

int grid_for(const msk_ctx* ctx, long items, long per_block) {
  long b = (items + per_block - 1) / per_block;
  const long cap = 16L * ctx->num_cu;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// lines of L entries: the widest power-of-two bundle of lines that fits the tile, at most 64 and at most what W needs
int tx_shift_for(int L, int W) {
  int s = 0;
  while (s < 6 && ((size_t)L << (s + 1)) * sizeof(double) <= (size_t)kTileBytes && (1 << s) < W) ++s;
  return s;
}

int launch_line(msk_ctx* ctx, const char* tag, double* g, int L, long lstride, int outer, long ostride, int W, double w) {
  if (L == 1) return 0;   // min over one entry with dy = 0: g + 0 = g
  const int s = tx_shift_for(L, W);
  const size_t lds = ((size_t)L << s) * sizeof(double) + ((size_t)1 << s) * sizeof(int);
  msk_launch_scope ls(ctx, tag);
  hipLaunchKernelGGL(edt_line_k, dim3((unsigned)((W + (1 << s) - 1) >> s), (unsigned)outer), dim3(kThreads), lds, ctx->stream,
                     g, L, lstride, ostride, W, s, w);
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // namespace

// the checks and the three passes of msk_edt3d; complement != 0: the features are {vol != cls} (msk_label_sdf of
// msk_loss_boundary.hip: the distance to the nearest voxel NOT of the class), surface_only must be 0 then
int msk_edt_field(msk_ctx* ctx, const int32_t* vol, int d, int h, int w, int cls, int surface_only, int complement,
                  const double* spacing, double* dist2) {
  if (int rc = check_volume(ctx, vol, d, h, w)) return rc;
  MSK_REQUIRE(ctx, dist2 != nullptr && (((uintptr_t)dist2) & 7) == 0, "dist2 must be an 8-byte aligned device pointer");
  MSK_REQUIRE(ctx, !(complement && surface_only), "the complemented transform has no surface form");
  double wgt[3] = {1.0, 1.0, 1.0};
  if (spacing != nullptr) {
    for (int a = 0; a < 3; ++a) {
      wgt[a] = spacing[a] * spacing[a];
      // w * 2047^2 * 3 must stay finite and w itself must not have left the normal range
      MSK_REQUIRE(ctx, spacing[a] > 0.0 && wgt[a] >= 1e-300 && wgt[a] <= 1e300, "spacing must be positive, its square within [1e-300, 1e300]");
    }
  }
  const Vol g{vol, d, h, w, cls, surface_only ? 1 : 0, complement ? 1 : 0};
  {
    msk_launch_scope ls(ctx, "edt_x");
    hipLaunchKernelGGL(edt_x_k, dim3((unsigned)grid_for(ctx, (long)d * h, kWaves)), dim3(kThreads), 0, ctx->stream, g, wgt[2], dist2);
    MSK_LAUNCH_CHECK(ctx);
  }
  if (int rc = launch_line(ctx, "edt_y", dist2, h, w, d, (long)h * w, w, wgt[1])) return rc;
  return launch_line(ctx, "edt_z", dist2, d, (long)h * w, h, w, w, wgt[0]);
}

extern "C" {

int msk_edt3d(msk_ctx* ctx, const int32_t* vol, int d, int h, int w, int cls, int surface_only, const double* spacing,
              double* dist2) {
  return msk_edt_field(ctx, vol, d, h, w, cls, surface_only, 0, spacing, dist2);
}

int msk_surface_count(msk_ctx* ctx, const int32_t* vol, int d, int h, int w, int cls, unsigned long long* count) {
  if (int rc = check_volume(ctx, vol, d, h, w)) return rc;
  MSK_REQUIRE(ctx, count != nullptr && (((uintptr_t)count) & 7) == 0, "count must be an 8-byte aligned device pointer");
  MSK_CHECK_HIP(ctx, hipMemsetAsync(count, 0, sizeof(unsigned long long), ctx->stream));
  const Vol g{vol, d, h, w, cls, 1, 0};
  msk_launch_scope ls(ctx, "surface_count");
  hipLaunchKernelGGL(surface_count_k, dim3((unsigned)grid_for(ctx, (long)d * h * w, 4L * kThreads)), dim3(kThreads), 0, ctx->stream,
                     g, count);
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

int msk_surface_gather(msk_ctx* ctx, const int32_t* vol, int d, int h, int w, int cls, const double* dist2, double* out,
                       long capacity, unsigned long long* count) {
  if (int rc = check_volume(ctx, vol, d, h, w)) return rc;
  MSK_REQUIRE(ctx, dist2 != nullptr && (((uintptr_t)dist2) & 7) == 0, "dist2 must be an 8-byte aligned device pointer");
  MSK_REQUIRE(ctx, capacity >= 0 && (out != nullptr || capacity == 0) && (((uintptr_t)out) & 7) == 0,
              "out must be an 8-byte aligned device pointer of `capacity` >= 0 doubles");
  MSK_REQUIRE(ctx, count != nullptr && (((uintptr_t)count) & 7) == 0, "count must be an 8-byte aligned device pointer");
  MSK_CHECK_HIP(ctx, hipMemsetAsync(count, 0, sizeof(unsigned long long), ctx->stream));
  const Vol g{vol, d, h, w, cls, 1, 0};
  msk_launch_scope ls(ctx, "surface_gather");
  hipLaunchKernelGGL(surface_gather_k, dim3((unsigned)grid_for(ctx, (long)d * h * w, 4L * kThreads)), dim3(kThreads), 0, ctx->stream,
                     g, dist2, out, capacity, count);
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
