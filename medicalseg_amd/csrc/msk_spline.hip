// Cubic B-spline resampling (functional.py:25-58 resize_3d, geometry.py:31-69 resample with order 3):
// scipy.ndimage.zoom(order=3, mode='nearest', grid_mode=False) as tests/spline_reference.py states it, bit for bit.
//
//   msk_spline_prefilter  the crop box, padded by kPad = 12 edge voxels per side, goes through the recursive B-spline
//                         prefilter along D, then H, then W, in float64, in a workspace of (sd+24)(sh+24)(sw+24) doubles.
//                         Per line c[0..n) with pole z = sqrt(3) - 2:
//                             c[i]   = gain * c[i]                          gain = (1 - z)(1 - 1/z)
//                             c[0]   = (c[0] + zn1 c[n-1] + sum_{i=1..min(n-2, 47)} z^i (c[i] + zn1 c[n-1-i])) * rden
//                             c[i]   = c[i] + z c[i-1]                      i = 1 .. n-1
//                             c[n-1] = last * (c[n-1] + z c[n-2])           last = z / (z z - 1)
//                             c[i]   = z * (c[i+1] - c[i])                  i = n-2 .. 0
//                         zn1 = z^(n-1) by repeated multiplication and rden = 1 / (1 - zn1 zn1) come from the host: the
//                         device neither raises to a power nor divides here.  z^i is the running product zi = zi * z.
//   msk_spline_zoom       one thread per output voxel, lanes along the output W: three weight quadruples in double around
//                         o * scale + 12 (scale = (n_in - 1) / (n_out - 1) from the host, 0 for one output voxel), the 64
//                         taps as acc = acc + ((p * wd) * wh) * ww with d outermost and w innermost, stored as float32.
//
// The D pass reads the float32 source with indices clamped to the BOX (the reference crops, then zooms), so the padded input
// is never materialised; the D and H passes give one line to a thread with the lanes along W, every access of a wavefront is
// one run of 512 bytes, and a thread fetches 16 samples of its line before it recurses over them, so 16 loads are in flight
// per lane (the recursion is a dependent chain: what hides the memory latency is the number of lines and this batch).  Along
// W a line is contiguous and a thread per line would stride by the line pitch, so a wavefront takes 64 lines through LDS, 48
// columns at a time: loaded row-wise (one 384-byte run per row), recursed column-wise (lane l walks row l, a whole chunk
// in registers), stored row-wise.  The recursion state (c[i-1], c[i-2] forward, c[i+1] backward) stays in registers from
// chunk to chunk; the last chunk of the forward sweep turns round in LDS, every other chunk is read again on the way back.
// The initialisation needs c[i] and c[n-1-i] together: it takes them through the same tile in two halves of 24 terms, 24
// columns of the head beside 24 of the tail.  So every pass is TWO round trips of the workspace through memory by
// construction (the forward sweep writes what the backward sweep reads), less the chunk that turns round on chip.  The one
// tile is 64 x 49 doubles = 24.5 KiB, six workgroups to a CU.  Its pitch of 49 doubles is odd: ds_read_b64 banks are
// (byte / 4) % 64 per 32-lane half, lane l of a column walk sits at dword 2 * 49 * l + const, and 98 l mod 64 takes 32
// distinct even values for l = 0..31: no two lanes on one bank.
//
// Everything is compiled under `#pragma clang fp contract(off)`: no multiply below may be fused with an add, on the device
// or on the host (the constants above are host arithmetic).  Indices are size_t.
#include <cmath>

#include "msk_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPad = 12;          // scipy's npad for mode='nearest'
constexpr int kHorizon = 47;      // terms of the initialisation sum: |z|^48 = 3.5e-28
constexpr int kThreads = 256;     // zoom
constexpr int kLineThreads = 64;  // D and H passes: one wavefront per workgroup, so that few lines still spread over the CUs
constexpr int kBatch = 16;        // D and H passes: samples fetched before the recursion runs over them
constexpr int kLines = 64;        // W pass: lines of a workgroup == its threads (one wavefront)
constexpr int kChunk = 48;        // W pass: columns in LDS at a time
constexpr int kPitch = kChunk + 1;
constexpr int kHalf = kChunk / 2; // W pass: terms of the initialisation per fill of the tile
static_assert(kHorizon + 1 == 2 * kHalf, "two fills of the tile cover c[0..kHorizon] and c[n-1-kHorizon..n-1]");
static_assert(kPitch % 2 == 1, "an odd pitch keeps the column walk of 8-byte elements off one bank");
static_assert(2 * kPad + 1 > kHalf, "the first fill's tail, c[n-kHalf..n-1], starts at c[1] or later");

struct SplineConst {
  double z, gain, last;
};
struct SplineAxis {
  double zn1, rden;   // z^(n-1), 1 / (1 - zn1 * zn1)
};
struct SplineBox {
  int fh, fw;         // row pitches of the whole volume
  int ci, cj, ck;     // box origin
  int sd, sh, sw;     // box extent
  int pd, ph, pw;     // padded extent
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One line whose samples the caller's `load(i)` yields already scaled by gain; written to line[i * stride].  load(i) may
// read line[i * stride] itself (in place): element i is written only after it was last read.
template <class Load>
__device__ __forceinline__ void filter_line(Load load, double* line, size_t stride, int n, const SplineConst& k,
                                            const SplineAxis& a) {
  const int last = n - 1;
  const int terms = min(n - 2, kHorizon);
  double zi = k.z;
  double c0 = load(0) + a.zn1 * load(last);
#pragma unroll 8
  for (int i = 1; i <= terms; ++i) {   // nothing is stored here: the loads of an unrolled body go out together
    c0 = c0 + zi * (load(i) + a.zn1 * load(last - i));
    zi = zi * k.z;
  }
  c0 = c0 * a.rden;
  line[0] = c0;
  double prev = c0, prev2 = c0;
  double v[kBatch];
  int i = 1;
  for (; i + kBatch <= n; i += kBatch) {
#pragma unroll
    for (int j = 0; j < kBatch; ++j) v[j] = load(i + j);
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const double x = v[j] + k.z * prev;
      line[(size_t)(i + j) * stride] = x;
      prev2 = prev;
      prev = x;
    }
  }
  for (; i < n; ++i) {
    const double x = load(i) + k.z * prev;
    line[(size_t)i * stride] = x;
    prev2 = prev;
    prev = x;
  }
  double next = k.last * (prev + k.z * prev2);
  line[(size_t)last * stride] = next;
  i = n - 2;
  for (; i - (kBatch - 1) >= 0; i -= kBatch) {
#pragma unroll
    for (int j = 0; j < kBatch; ++j) v[j] = line[(size_t)(i - j) * stride];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const double x = k.z * (next - v[j]);
      line[(size_t)(i - j) * stride] = x;
      next = x;
    }
  }
  for (; i >= 0; --i) {
    const double x = k.z * (next - line[(size_t)i * stride]);
    line[(size_t)i * stride] = x;
    next = x;
  }
}

// D pass: thread = (hp, wp) of the padded box, the line runs along D; reads the float32 source, clamped to the box
__global__ void __launch_bounds__(kLineThreads)
spline_pass_d_k(const float* __restrict__ src, double* __restrict__ ws, SplineBox g, SplineConst k, SplineAxis a) {
  const size_t plane = (size_t)g.ph * g.pw;
  const size_t t = (size_t)blockIdx.x * kLineThreads + threadIdx.x;
  if (t >= plane) return;
  const int hp = (int)(t / (size_t)g.pw), wp = (int)(t - (size_t)hp * g.pw);
  const int h = clampi(hp - kPad, g.sh - 1) + g.cj, w = clampi(wp - kPad, g.sw - 1) + g.ck;
  const size_t fplane = (size_t)g.fh * g.fw;
  const float* __restrict__ col = src + (size_t)g.ci * fplane + (size_t)h * g.fw + w;
  const int sd1 = g.sd - 1;
  const double gain = k.gain;
  filter_line([&](int i) { return gain * (double)col[(size_t)clampi(i - kPad, sd1) * fplane]; }, ws + t, plane, g.pd, k, a);
}

// H pass: thread = (dp, wp), the line runs along H, in place
__global__ void __launch_bounds__(kLineThreads)
spline_pass_h_k(double* __restrict__ ws, SplineBox g, SplineConst k, SplineAxis a) {
  const size_t lines = (size_t)g.pd * g.pw;
  const size_t t = (size_t)blockIdx.x * kLineThreads + threadIdx.x;
  if (t >= lines) return;
  const int dp = (int)(t / (size_t)g.pw), wp = (int)(t - (size_t)dp * g.pw);
  double* line = ws + (size_t)dp * g.ph * g.pw + wp;
  const size_t stride = (size_t)g.pw;
  const double gain = k.gain;
  filter_line([&](int i) { return gain * line[(size_t)i * stride]; }, line, stride, g.ph, k, a);
}

// columns [c0, c0 + nc) of rows [r0, r0 + nl) <-> the tile; one 8 * nc byte run per row
template <bool kScaled>
__device__ __forceinline__ void tile_in(const double* __restrict__ ws, size_t r0, int nl, size_t n, int c0, int nc, double gain,
                                        double* tile) {
  const int t = threadIdx.x;
  if (t < nc) {
    const double* __restrict__ p = ws + r0 * n + c0 + t;
#pragma unroll 8
    for (int r = 0; r < nl; ++r) {
      const double v = p[(size_t)r * n];
      tile[r * kPitch + t] = kScaled ? gain * v : v;
    }
  }
}
__device__ __forceinline__ void tile_out(double* __restrict__ ws, size_t r0, int nl, size_t n, int c0, int nc, const double* tile) {
  const int t = threadIdx.x;
  if (t < nc) {
    double* __restrict__ p = ws + r0 * n + c0 + t;
#pragma unroll 8
    for (int r = 0; r < nl; ++r) p[(size_t)r * n] = tile[r * kPitch + t];
  }
}
// one fill for the initialisation, scaled: tile columns [0, kHalf) = c[hbase ..], columns [kHalf, kChunk) = c[tbase ..];
// a column outside the line is not loaded (and not read: the sum stops at c[n-2] and c[1])
__device__ __forceinline__ void tile_in_halves(const double* __restrict__ ws, size_t r0, int nl, int n, int hbase, int tbase,
                                               double gain, double* tile) {
  const int t = threadIdx.x;
  const int c = t < kHalf ? hbase + t : tbase + (t - kHalf);
  if (t < kChunk && c >= 0 && c < n) {
    const double* __restrict__ p = ws + r0 * (size_t)n + c;
#pragma unroll 8
    for (int r = 0; r < nl; ++r) tile[r * kPitch + t] = gain * p[(size_t)r * n];
  }
}

// W pass: a wavefront owns kLines rows of the workspace (a row = one line along W), in place
__global__ void __launch_bounds__(kLines)
spline_pass_w_k(double* __restrict__ ws, size_t rows, int n, SplineConst k, SplineAxis a) {
  __shared__ double tile[kLines * kPitch];
  const int t = threadIdx.x;
  const size_t r0 = (size_t)blockIdx.x * kLines;
  const int nl = (int)min((size_t)kLines, rows - r0);
  const bool mine = t < nl;
  const int last = n - 1;
  const int nchunks = (n + kChunk - 1) / kChunk;
  const int terms = min(n - 2, kHorizon);
  double* row = tile + t * kPitch;

  // the initialisation: terms 0 .. kHalf-1 from c[0 .. kHalf) and c[n-kHalf .. n), then terms kHalf .. 2 kHalf - 1 from
  // c[kHalf .. 2 kHalf) and c[n - 2 kHalf .. n - kHalf); term i pairs tile column i (mod kHalf) with column kChunk - 1 - i
  double c0 = 0.0, zi = k.z;
  tile_in_halves(ws, r0, nl, n, 0, n - kHalf, k.gain, tile);
  __syncthreads();
  if (mine) {
    c0 = row[0] + a.zn1 * row[kChunk - 1];
    const int stop = min(terms, kHalf - 1);
    for (int i = 1; i <= stop; ++i) {
      c0 = c0 + zi * (row[i] + a.zn1 * row[kChunk - 1 - i]);
      zi = zi * k.z;
    }
  }
  if (terms >= kHalf) {   // the same for every thread
    __syncthreads();
    tile_in_halves(ws, r0, nl, n, kHalf, n - 2 * kHalf, k.gain, tile);
    __syncthreads();
    if (mine)
      for (int i = kHalf; i <= terms; ++i) {
        c0 = c0 + zi * (row[i - kHalf] + a.zn1 * row[kChunk - 1 - (i - kHalf)]);
        zi = zi * k.z;
      }
  }
  c0 = c0 * a.rden;
  double prev = c0, prev2 = c0, next = 0.0;
  double v[kChunk];
  for (int ch = 0; ch < nchunks; ++ch) {
    const int cb = ch * kChunk, nc = min(kChunk, n - cb);
    __syncthreads();   // the tile was read: by the initialisation, or by the store of the chunk before
    tile_in<true>(ws, r0, nl, (size_t)n, cb, nc, k.gain, tile);
    __syncthreads();
    if (mine) {
      if (ch == 0) row[0] = c0;
      if (nc == kChunk && ch > 0 && ch < nchunks - 1) {   // a whole chunk in registers, then the chain
#pragma unroll
        for (int j = 0; j < kChunk; ++j) v[j] = row[j];
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
          const double x = v[j] + k.z * prev;
          row[j] = x;
          prev2 = prev;
          prev = x;
        }
      } else {
        for (int j = ch == 0 ? 1 : 0; j < nc; ++j) {
          const double x = row[j] + k.z * prev;
          row[j] = x;
          prev2 = prev;
          prev = x;
        }
        if (ch == nchunks - 1) {   // the last chunk turns round on chip
          next = k.last * (prev + k.z * prev2);
          row[nc - 1] = next;
          for (int j = nc - 2; j >= 0; --j) {
            const double x = k.z * (next - row[j]);
            row[j] = x;
            next = x;
          }
        }
      }
    }
    __syncthreads();
    tile_out(ws, r0, nl, (size_t)n, cb, nc, tile);
  }
  for (int ch = nchunks - 2; ch >= 0; --ch) {
    const int cb = ch * kChunk;
    __syncthreads();
    tile_in<false>(ws, r0, nl, (size_t)n, cb, kChunk, 1.0, tile);
    __syncthreads();
    if (mine) {
#pragma unroll
      for (int j = 0; j < kChunk; ++j) v[j] = row[kChunk - 1 - j];
#pragma unroll
      for (int j = 0; j < kChunk; ++j) {
        const double x = k.z * (next - v[j]);
        row[kChunk - 1 - j] = x;
        next = x;
      }
    }
    __syncthreads();
    tile_out(ws, r0, nl, (size_t)n, cb, kChunk, tile);
  }
}

struct ZoomArgs {
  int pd, ph, pw;
  int dd, dh, dw;
  double scale_d, scale_h, scale_w;
};

// first tap and the four weights of output index o
__device__ __forceinline__ int spline_weights(int o, double scale, int p, double (&w)[4]) {
  const double cc = (double)o * scale + (double)kPad;
  const double f = floor(cc);
  const double t = cc - f, u = 1.0 - t;
  w[0] = ((u * u) * u) / 6.0;
  w[1] = (((t * t) * (t - 2.0)) * 3.0 + 4.0) / 6.0;
  w[2] = (((u * u) * (u - 2.0)) * 3.0 + 4.0) / 6.0;
  w[3] = ((1.0 - w[0]) - w[1]) - w[2];
  // 11 <= start and start + 3 <= n_in + 13 < p by the coordinate map; the clamp keeps a rounding accident inside the workspace
  return clampi((int)f - 1, p - 4);
}

__global__ void __launch_bounds__(kThreads)
spline_zoom_k(const double* __restrict__ ws, float* __restrict__ dst, ZoomArgs g) {
  const size_t total = (size_t)g.dd * g.dh * g.dw;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const int ow = (int)(i % (size_t)g.dw);
    const int oh = (int)((i / (size_t)g.dw) % (size_t)g.dh);
    const int od = (int)(i / ((size_t)g.dw * g.dh));
    double wd[4], wh[4], ww[4];
    const int sd = spline_weights(od, g.scale_d, g.pd, wd);
    const int sh = spline_weights(oh, g.scale_h, g.ph, wh);
    const int sw = spline_weights(ow, g.scale_w, g.pw, ww);
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const double* __restrict__ p = ws + ((size_t)(sd + a) * g.ph + (size_t)(sh + b)) * g.pw + sw;
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = acc + ((p[c] * wd[a]) * wh[b]) * ww[c];
      }
    dst[i] = (float)acc;
  }
}

inline bool padded_ok(int sd, int sh, int sw) {
  const long lim = 0x7fffffffL - 2 * kPad;
  if (sd < 1 || sh < 1 || sw < 1 || sd > lim || sh > lim || sw > lim) return false;
  const unsigned long long pd = (unsigned long long)sd + 2 * kPad, ph = (unsigned long long)sh + 2 * kPad, pw = (unsigned long long)sw + 2 * kPad;
  // pd * ph < 2^62, and the quotient keeps the triple product below 2^31 without forming it
  return pd * ph <= 0x7fffffffULL && pw <= 0x7fffffffULL / (pd * ph);
}

inline SplineAxis axis_const(int n, double z) {
  double zn1 = 1.0;
  for (int i = 0; i < n - 1; ++i) zn1 = zn1 * z;
  SplineAxis a;
  a.zn1 = zn1;
  a.rden = 1.0 / (1.0 - zn1 * zn1);
  return a;
}

inline double axis_scale(int n_in, int n_out) { return n_out > 1 ? (double)(n_in - 1) / (double)(n_out - 1) : 0.0; }

}  // namespace

extern "C" {

int msk_spline_workspace(int sd, int sh, int sw, size_t* bytes) {
  MSK_REQUIRE(nullptr, bytes != nullptr, "bytes must not be null");
  MSK_REQUIRE(nullptr, padded_ok(sd, sh, sw), "extents must be >= 1 and the padded box (+24 per axis) must have fewer than 2^31 voxels");
  const size_t doubles = (size_t)(sd + 2 * kPad) * (size_t)(sh + 2 * kPad) * (size_t)(sw + 2 * kPad);
  *bytes = (doubles * sizeof(double) + 255) & ~(size_t)255;
  return 0;
}

int msk_spline_resample3d(msk_ctx* ctx, const float* src, int fd, int fh, int fw, int ci, int cj, int ck, int sd, int sh, int sw,
                          float* dst, int dd, int dh, int dw, void* work, size_t work_bytes) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, src != nullptr && dst != nullptr && work != nullptr, "null src / dst / work");
  MSK_REQUIRE(ctx, fd > 0 && fh > 0 && fw > 0 && sd > 0 && sh > 0 && sw > 0 && dd > 0 && dh > 0 && dw > 0, "empty volume");
  MSK_REQUIRE(ctx, ci >= 0 && cj >= 0 && ck >= 0 && (long)ci + sd <= fd && (long)cj + sh <= fh && (long)ck + sw <= fw,
              "crop box outside the volume");
  MSK_REQUIRE(ctx, msk_below_2_31(fd, fh, fw) && msk_below_2_31(dd, dh, dw) && padded_ok(sd, sh, sw),
              "volume, destination and padded box must have fewer than 2^31 voxels each");
  MSK_REQUIRE(ctx, (((uintptr_t)src | (uintptr_t)dst) & 3) == 0 && (((uintptr_t)work) & 7) == 0,
              "src / dst must be 4-byte aligned, work 8-byte aligned");
  SplineBox g;
  g.fh = fh; g.fw = fw;
  g.ci = ci; g.cj = cj; g.ck = ck;
  g.sd = sd; g.sh = sh; g.sw = sw;
  g.pd = sd + 2 * kPad; g.ph = sh + 2 * kPad; g.pw = sw + 2 * kPad;
  const size_t need = (size_t)g.pd * g.ph * g.pw * sizeof(double);
  MSK_REQUIRE(ctx, work_bytes >= need, "workspace smaller than msk_spline_workspace(sd, sh, sw)");
  const size_t vbytes = (size_t)fd * fh * fw * 4, obytes = (size_t)dd * dh * dw * 4;
  MSK_REQUIRE(ctx, msk_bytes_disjoint(dst, obytes, src, vbytes) && msk_bytes_disjoint(work, need, src, vbytes) &&
                       msk_bytes_disjoint(work, need, dst, obytes), "src, dst and work must not overlap");
  SplineConst k;
  k.z = sqrt(3.0) - 2.0;
  k.gain = (1.0 - k.z) * (1.0 - 1.0 / k.z);
  k.last = k.z / (k.z * k.z - 1.0);
  double* ws = (double*)work;
  {
    msk_launch_scope ls(ctx, "spline_prefilter_d");
    hipLaunchKernelGGL(spline_pass_d_k, dim3((unsigned)msk_cdiv((long)g.ph * g.pw, kLineThreads)), dim3(kLineThreads), 0, ctx->stream, src, ws,
                       g, k, axis_const(g.pd, k.z));
  }
  MSK_LAUNCH_CHECK(ctx);
  {
    msk_launch_scope ls(ctx, "spline_prefilter_h");
    hipLaunchKernelGGL(spline_pass_h_k, dim3((unsigned)msk_cdiv((long)g.pd * g.pw, kLineThreads)), dim3(kLineThreads), 0, ctx->stream, ws, g, k,
                       axis_const(g.ph, k.z));
  }
  MSK_LAUNCH_CHECK(ctx);
  {
    const size_t rows = (size_t)g.pd * g.ph;
    msk_launch_scope ls(ctx, "spline_prefilter_w");
    hipLaunchKernelGGL(spline_pass_w_k, dim3((unsigned)msk_cdiv((long)rows, kLines)), dim3(kLines), 0, ctx->stream, ws, rows, g.pw, k,
                       axis_const(g.pw, k.z));
  }
  MSK_LAUNCH_CHECK(ctx);
  ZoomArgs za;
  za.pd = g.pd; za.ph = g.ph; za.pw = g.pw;
  za.dd = dd; za.dh = dh; za.dw = dw;
  za.scale_d = axis_scale(sd, dd);
  za.scale_h = axis_scale(sh, dh);
  za.scale_w = axis_scale(sw, dw);
  {
    msk_launch_scope ls(ctx, "spline_zoom");
    hipLaunchKernelGGL(spline_zoom_k, dim3((unsigned)msk_ew_blocks((long)dd * dh * dw, ctx->num_cu)), dim3(kThreads), 0, ctx->stream,
                       (const double*)ws, dst, za);
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
