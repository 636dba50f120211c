// The displacement field of the elastic deformation (transforms.RandomElasticAffinePatchCrop3D, tests/elastic_reference.py):
// three components of uniform noise in [-1, 1) from the counter RNG, each smoothed by a wide Gaussian (sigma up to 16, radius
// r = int(4 sigma + 0.5) up to 64) along W, then H, then D with zeros outside the patch (scipy's mode='constant'), times alpha.
// It replaces batchgenerators' elastic_deform_coordinates, which is not in the reference.  msk_affine_patch_elastic
// (msk_affine.hip) adds the field to the sampling grid in front of the matrix.
//
// Per line acc = w[0]*x[i-r], then acc = acc + w[k]*x[i-r+k] for k = 1..2r: all 2r+1 terms, an operand outside the line is
// +0.0, every multiply and add rounded on its own (`#pragma clang fp contract(off)`), so the field equals the numpy statement
// bit for bit and two calls give the same bits.  No atomics, no synchronisation, no download.
//
// Radius 64 does not fit the register form of msk_intensity.hip's blur (16 + 2r operands per thread).  Here a thread owns
// kOut = 8 consecutive outputs of its line and walks the 2r+1 taps with a window of 16 operands in registers: eight new
// operands per eight taps, so one operand load feeds eight multiply-adds and the passes are bound by the vector ALU
// (2 operations per tap and output), not by operand traffic.
//   W pass  a workgroup covers up to 32 rows x a segment of S = 8 * (threads per row) <= 256 columns.  The segment plus r
//           operands on either side is GENERATED into LDS from the counter (no noise buffer exists); a column outside the row
//           is stored as +0.0 from a predicate.  The generation costs (S + 2r) / S splitmix64 words per output against 2r+1
//           taps.  A thread reads its window with two 16-byte LDS loads per eight taps (2-way bank conflict between lanes l and
//           l+8 of a row, which the ALU work hides: 16 LDS cycles against 128 vector instructions).
//   H, D    the volume as [outer][L][inner]: a thread owns one (outer, inner) column and 8 outputs along L; lanes are
//           consecutive addresses of the contiguous axis, so every load is a coalesced line, and an operand outside the line is
//           +0.0 from a predicate (the load is not issued).  A pass re-reads (2r + 8) / 8 of the field from L2.
//   A component whose axis is not requested is +0.0 everywhere: it is cleared and takes part in no pass.
#include "msk_common.h"

#pragma clang fp contract(off)   // for the whole file: every multiply and add below is rounded on its own

namespace {

constexpr int kThreads = 256;
constexpr int kMaxR = 64;
constexpr int kMinR = 2;
constexpr int kOut = 8;               // consecutive outputs per thread
constexpr int kMaxExtent = 8192;
constexpr float kMaxAlpha = 4096.0f;
constexpr int kMaxRows = 32;          // rows per workgroup of the W pass
constexpr int kMaxTpr = 32;           // threads per row segment: S <= 256
constexpr int kLdsFloats = 6400;      // covers every (threads per row, r): see row_stride / the static_asserts below

// LDS line of the W pass: the segment, r operands on either side, and the 8 the last window step loads beyond what it uses;
// rounded up so that every line starts 16-byte aligned
constexpr int row_stride(int tpr, int r) { return (tpr * kOut + 2 * r + kOut + 3) & ~3; }
constexpr int rows_of(int tpr) { return kThreads / tpr < kMaxRows ? kThreads / tpr : kMaxRows; }
constexpr bool lds_fits() {
  for (int tpr = 1; tpr <= kMaxTpr; ++tpr)
    if (rows_of(tpr) * row_stride(tpr, kMaxR) > kLdsFloats) return false;
  return true;
}
static_assert(lds_fits(), "the W pass tile must fit its LDS array for every row length");

struct FieldArgs {
  int rd, rh, rw;
  int r;
  int ncomp;
  int comp[3];      // the requested components, ascending
  uint64_t key;     // splitmix64(seed)
  float alpha;
  float w[2 * kMaxR + 1];
};

// acc[j] = sum over k = 0..2r ascending of w[k] * op(k + j), j = 0..7, starting from the first product.  load(dst, j0) puts the
// operands op(j0) .. op(j0 + 7) into dst; it is called for j0 = 0, 8, .., the last one up to 8 past 2r + 7 (values unused).
template <class Load>
__device__ __forceinline__ void filter8(const Load& load, const float* __restrict__ w, int r, float (&acc)[kOut]) {
  float win[2 * kOut];
  load(win, 0);
#pragma unroll
  for (int j = 0; j < kOut; ++j) acc[j] = w[0] * win[j];
  const int last = 2 * r;
  for (int kk = 0; kk < last; kk += kOut) {    // taps kk+1 .. kk+8; win[0] = op(kk)
    load(win + kOut, kk + kOut);
#pragma unroll
    for (int u = 1; u <= kOut; ++u) {
      if (kk + u <= last) {                    // the same in every thread
        const float wk = w[kk + u];
#pragma unroll
        for (int j = 0; j < kOut; ++j) acc[j] = acc[j] + wk * win[u + j];
      }
    }
#pragma unroll
    for (int j = 0; j < kOut; ++j) win[j] = win[j + kOut];
  }
}

// W pass.  blockIdx.x = tile of `rows` rows of the requested components ([ncomp][rd*rh] rows), blockIdx.y = segment of tpr*8
// columns.  Offsets are 32-bit: 3 * rd*rh*rw < 2^31.
__global__ void __launch_bounds__(kThreads)
field_row_k(float* __restrict__ dst, const FieldArgs g, int tpr, int rows, int stride) {
  __shared__ __attribute__((aligned(16))) float tile[kLdsFloats];
  const int t = threadIdx.x;
  const int rows_per_comp = g.rd * g.rh;
  const int rows_total = g.ncomp * rows_per_comp;
  const int n = rows_per_comp * g.rw;
  const int row0 = (int)blockIdx.x * rows;
  const int seg0 = (int)blockIdx.y * tpr * kOut;
  const int nrows = rows_total - row0 < rows ? rows_total - row0 : rows;
  const int line = tpr * kOut + 2 * g.r + kOut;       // <= stride
  for (int e = t; e < nrows * line; e += kThreads) {
    const int lr = e / line, j = e - lr * line;
    const int x = seg0 - g.r + j;
    float v = 0.f;
    if ((unsigned)x < (unsigned)g.rw) {
      const int row = row0 + lr;
      const int ci = row / rows_per_comp, rr = row - ci * rows_per_comp;
      const uint64_t idx = (uint64_t)g.comp[ci] * (uint64_t)n + (uint64_t)(rr * g.rw + x);
      const uint64_t h = splitmix64(g.key + idx);
      v = (float)(uint32_t)(h >> 40) * 0x1p-23f - 1.0f;   // exact: a multiple of 2^-23 in [-1, 1)
    }
    tile[lr * stride + j] = v;
  }
  __syncthreads();
  const int lr = t / tpr, q = t - lr * tpr;
  if (lr >= nrows) return;
  const int x0 = seg0 + q * kOut;
  if (x0 >= g.rw) return;
  const float* p = tile + lr * stride + q * kOut;     // p[k + j]: the operand of tap k of output x0 + j; 16-byte aligned
  float acc[kOut];
  filter8([p](float* d, int j0) {
    const float4 a = *reinterpret_cast<const float4*>(p + j0), b = *reinterpret_cast<const float4*>(p + j0 + 4);
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
  }, g.w, g.r, acc);
  const int row = row0 + lr;
  const int ci = row / rows_per_comp, rr = row - ci * rows_per_comp;
  float* out = dst + g.comp[ci] * n + rr * g.rw + x0;
#pragma unroll
  for (int j = 0; j < kOut; ++j)
    if (x0 + j < g.rw) out[j] = acc[j];
}

// H and D passes: every requested component as [outer][L][inner], filtered along L.  thread: one (component, outer, inner)
// column, 8 outputs from blockIdx.y * 8.  kScale: the last pass multiplies by alpha.
template <bool kScale>
__global__ void __launch_bounds__(kThreads)
field_column_k(const float* __restrict__ src, float* __restrict__ dst, const FieldArgs g, int outer, int L, int inner) {
  const int per_comp = outer * inner;
  const int col = (int)blockIdx.x * kThreads + threadIdx.x;
  if (col >= g.ncomp * per_comp) return;
  const int ci = col / per_comp, rest = col - ci * per_comp;
  const int o = rest / inner, c = rest - o * inner;
  const int base = g.comp[ci] * (per_comp * L) + o * L * inner + c;
  const int i0 = (int)blockIdx.y * kOut;
  const float* q = src + base;
  const int first = i0 - g.r;
  float acc[kOut];
  filter8([q, first, L, inner](float* d, int j0) {
#pragma unroll
    for (int j = 0; j < kOut; ++j) {
      const int li = first + j0 + j;
      d[j] = (unsigned)li < (unsigned)L ? q[li * inner] : 0.f;    // outside the line: no load
    }
  }, g.w, g.r, acc);
  float* out = dst + base + i0 * inner;
#pragma unroll
  for (int j = 0; j < kOut; ++j)
    if (i0 + j < L) out[j * inner] = kScale ? g.alpha * acc[j] : acc[j];
}

}  // namespace

extern "C" {

int msk_elastic_field(msk_ctx* ctx, uint64_t seed, int rd, int rh, int rw, const float* taps, int r, float alpha, int axes_mask,
                      float* field, float* scratch) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, taps != nullptr && field != nullptr && scratch != nullptr, "null taps / field / scratch");
  MSK_REQUIRE(ctx, r >= kMinR && r <= kMaxR, "r must be in [2, 64]");
  // written so that a NaN fails
  MSK_REQUIRE(ctx, alpha >= 0.0f && alpha <= kMaxAlpha, "alpha must be finite and inside [0, 4096]");
  MSK_REQUIRE(ctx, axes_mask >= 0 && axes_mask <= 7, "axes_mask must be a subset of bits 0..2");
  MSK_REQUIRE(ctx, rd >= 1 && rh >= 1 && rw >= 1 && rd <= kMaxExtent && rh <= kMaxExtent && rw <= kMaxExtent,
              "patch extents must be in [1, 8192]");
  const long n = (long)rd * rh * rw;
  MSK_REQUIRE(ctx, 3 * n <= 0x7fffffffL, "the field must have fewer than 2^31 elements");
  MSK_REQUIRE(ctx, ((((uintptr_t)field) | ((uintptr_t)scratch)) & 3) == 0, "field / scratch must be 4-byte aligned");
  const size_t bytes = (size_t)n * 12;
  MSK_REQUIRE(ctx, msk_bytes_disjoint(field, bytes, scratch, bytes), "field must not overlap scratch");
  FieldArgs g;
  g.rd = rd; g.rh = rh; g.rw = rw;
  g.r = r;
  g.ncomp = 0;
  g.comp[0] = g.comp[1] = g.comp[2] = 0;
  for (int a = 0; a < 3; ++a)
    if (axes_mask & (1 << a)) g.comp[g.ncomp++] = a;
  g.key = splitmix64(seed);
  g.alpha = alpha;
  for (int k = 0; k <= 2 * r; ++k) {
    MSK_REQUIRE(ctx, taps[k] >= 0.0f && taps[k] <= 1.0f, "taps must be finite and inside [0, 1]");
    g.w[k] = taps[k];
  }
  for (int k = 2 * r + 1; k <= 2 * kMaxR; ++k) g.w[k] = 0.f;
  msk_launch_scope ls(ctx, "elastic_field");
  for (int a = 0; a < 3; ++a)   // a component that is not requested: +0.0 everywhere
    if (!(axes_mask & (1 << a))) MSK_CHECK_HIP(ctx, hipMemsetAsync(field + (size_t)a * n, 0, (size_t)n * 4, ctx->stream));
  if (g.ncomp == 0) return 0;
  const int tpr = msk_cdiv(rw < kMaxTpr * kOut ? rw : kMaxTpr * kOut, kOut);
  const int rows = rows_of(tpr);
  const long rows_total = (long)g.ncomp * rd * rh;
  // grid.x < 2^31 / 8, grid.y <= 8192 / 8
  hipLaunchKernelGGL(field_row_k, dim3((unsigned)msk_cdiv(rows_total, rows), (unsigned)msk_cdiv(rw, tpr * kOut)), dim3(kThreads), 0,
                     ctx->stream, field, g, tpr, rows, row_stride(tpr, r));
  hipLaunchKernelGGL(field_column_k<false>, dim3((unsigned)msk_cdiv((long)g.ncomp * rd * rw, kThreads), (unsigned)msk_cdiv(rh, kOut)),
                     dim3(kThreads), 0, ctx->stream, field, scratch, g, rd, rh, rw);
  hipLaunchKernelGGL(field_column_k<true>, dim3((unsigned)msk_cdiv((long)g.ncomp * rh * rw, kThreads), (unsigned)msk_cdiv(rd, kOut)),
                     dim3(kThreads), 0, ctx->stream, scratch, field, g, 1, rd, rh * rw);
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
