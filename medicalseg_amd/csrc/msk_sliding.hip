// Sliding-window inference (core/infer.py sliding_window_inference): crop windows out of a volume with implicit padding, and add a
// window's logits, weighted per voxel, into the whole-volume accumulator.  The kernels only stream: no LDS, no atomics.  One
// launch per window on the context stream, so the windows of one call that overlap are added in window order.  The mirrored
// entry points (msk_sw_gather_mirrored / msk_sw_accumulate_mirrored: nnU-Net's mirroring inside the sliding window) take a mask
// per window pass (bit 0 = D, bit 1 = H, bit 2 = W, about the WINDOW); the accumulate adds the up to 8 passes of one window in
// one launch: the accumulator is read and written once, every pass's logits once at their mirrored addresses.
// Every product is rounded to fp32 before it is added (rn_mul / rn_add below): the results are pinned bit for bit against
// numpy float32 (tests/sliding_reference.py, tests/sliding_mirror_reference.py), and an FMA differs from it in the last bit
// wherever two windows overlap.
// __fmul_rn / __fadd_rn do NOT guarantee that here: in this toolchain they are inline `x * y` / `x + y` of a header compiled
// with the default contract = fast, and `__fadd_rn(acc, __fmul_rn(w, l))` came out as one v_fma_f32.  The two helpers are
// the same operators compiled under `#pragma clang fp contract(off)`, which the backend then may not fuse.
//
// Thread-to-element map: a window clipped to the volume is a set of W rows, each one contiguous run of floats in the window
// tensor and in the volume.  Where both tensors are dense and every row starts on and is a whole number of 16-byte quads, a
// thread owns one quad (consecutive lanes consecutive quads of a row, 1 KiB per wavefront instruction whatever C is); otherwise
// (channel-slice views, odd row starts or lengths) a thread owns one float, consecutive lanes consecutive floats of a row.
#include "msk_common.h"

#include <climits>

#pragma clang fp contract(off)   // for the whole file: no multiply below may be fused with an add

namespace {

__device__ __forceinline__ float rn_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float rn_add(float a, float b) { return a + b; }

constexpr int kThreads = 256;

struct SwBox {      // one window: origin in volume coordinates and the part of it that lies inside the volume (window-local)
  int n, d0, h0, w0;
  int z0, nz, y0, ny, x0, nx;
};

struct SwDims {
  int D, H, W;      // volume extent
  int rd, rh, rw;   // window extent
  int C;
};

// patch quad <- volume quad or cval.  Threads cover the WHOLE window (the padding is written too).  mask mirrors the patch
// about the window: bits 0 / 1 remap whole rows; bit 2 (the host sends it here for C == 1 only) takes the row's mirrored quad
// and reverses it in registers.
template <typename I>
__global__ void __launch_bounds__(kThreads)
sw_gather_quad_k(const float* __restrict__ vol, float* __restrict__ patch, SwDims g, SwBox b, float cval, int src_quads, int mask) {
  const int rq = g.rw * g.C >> 2;
  const long total = (long)g.rd * g.rh * rq;
  const long li = (long)blockIdx.x * kThreads + threadIdx.x;
  if (li >= total) return;
  const I i = (I)li;
  const I r = i / (I)rq;
  const int q = (int)(i - r * (I)rq);
  const int z = (int)(r / (I)g.rh), y = (int)(r - (I)z * (I)g.rh);
  const int d = b.d0 + (mask & 1 ? g.rd - 1 - z : z), h = b.h0 + (mask & 2 ? g.rh - 1 - y : y);
  const bool row_ok = d >= 0 && d < g.D && h >= 0 && h < g.H;
  const long rowlen = (long)g.W * g.C;
  const long s = (long)b.w0 * g.C + 4L * (mask & 4 ? rq - 1 - q : q);   // first float of the quad inside the volume row (may be < 0)
  const float* src = vol + (((long)b.n * g.D + d) * g.H + h) * rowlen;   // dereferenced only where row_ok
  float4 v = make_float4(cval, cval, cval, cval);
  if (row_ok) {
    if (src_quads && s >= 0 && s + 3 < rowlen) {
      v = *reinterpret_cast<const float4*>(src + s);
    } else {
      if (s >= 0 && s < rowlen) v.x = src[s];
      if (s + 1 >= 0 && s + 1 < rowlen) v.y = src[s + 1];
      if (s + 2 >= 0 && s + 2 < rowlen) v.z = src[s + 2];
      if (s + 3 >= 0 && s + 3 < rowlen) v.w = src[s + 3];
    }
  }
  if (mask & 4) v = make_float4(v.w, v.z, v.y, v.x);
  reinterpret_cast<float4*>(patch)[li] = v;
}

// any ld, any extents: one thread per float of the window
template <typename I>
__global__ void __launch_bounds__(kThreads)
sw_gather_elem_k(const float* __restrict__ vol, int vld, float* __restrict__ patch, int pld, SwDims g, SwBox b, float cval, int mask) {
  const long total = (long)g.rd * g.rh * g.rw * g.C;
  const long li = (long)blockIdx.x * kThreads + threadIdx.x;
  if (li >= total) return;
  const I i = (I)li;
  const I v = i / (I)g.C;
  const int c = (int)(i - v * (I)g.C);
  const I r = v / (I)g.rw;
  const int x = (int)(v - r * (I)g.rw);
  const int z = (int)(r / (I)g.rh), y = (int)(r - (I)z * (I)g.rh);
  const int d = b.d0 + (mask & 1 ? g.rd - 1 - z : z), h = b.h0 + (mask & 2 ? g.rh - 1 - y : y), w = b.w0 + (mask & 4 ? g.rw - 1 - x : x);
  float val = cval;
  if (d >= 0 && d < g.D && h >= 0 && h < g.H && w >= 0 && w < g.W) val = vol[((((long)b.n * g.D + d) * g.H + h) * g.W + w) * vld + c];
  patch[(long)v * pld + c] = val;
}

// acc quad += weight * logits quad, over the part of the window inside the volume; rows are whole quads in both tensors
template <typename I>
__global__ void __launch_bounds__(kThreads)
sw_acc_quad_k(const float* __restrict__ logits, float* __restrict__ acc, const float* __restrict__ td, const float* __restrict__ th,
              const float* __restrict__ tw, SwDims g, SwBox b) {
  const int rq = b.nx * g.C >> 2;
  const long total = (long)b.nz * b.ny * rq;
  const long li = (long)blockIdx.x * kThreads + threadIdx.x;
  if (li >= total) return;
  const I i = (I)li;
  const I r = i / (I)rq;
  const int q = (int)(i - r * (I)rq);
  const int zi = (int)(r / (I)b.ny);
  const int z = b.z0 + zi, y = b.y0 + (int)(r - (I)zi * (I)b.ny);
  const float wzy = rn_mul(td[z], th[y]);
  const long lo = (((long)z * g.rh + y) * g.rw + b.x0) * g.C + 4L * q;
  const long ao = ((((long)b.n * g.D + b.d0 + z) * g.H + b.h0 + y) * g.W + b.w0 + b.x0) * g.C + 4L * q;
  const float4 l = *reinterpret_cast<const float4*>(logits + lo);
  float4 a = *reinterpret_cast<const float4*>(acc + ao);
  int xo = (4 * q) / g.C;                                        // voxel of the quad's first float, from x0
  int rem = 4 * q - xo * g.C;                                    // its channel
  const float* t = tw + b.x0;
  float w = rn_mul(wzy, t[xo]);
  a.x = rn_add(a.x, rn_mul(w, l.x));
  if (++rem == g.C) { rem = 0; w = rn_mul(wzy, t[++xo]); }
  a.y = rn_add(a.y, rn_mul(w, l.y));
  if (++rem == g.C) { rem = 0; w = rn_mul(wzy, t[++xo]); }
  a.z = rn_add(a.z, rn_mul(w, l.z));
  if (++rem == g.C) { rem = 0; w = rn_mul(wzy, t[++xo]); }   // the quad's last float is inside the row: xo < nx
  a.w = rn_add(a.w, rn_mul(w, l.w));
  *reinterpret_cast<float4*>(acc + ao) = a;
}

// any ld, any extents: one thread per float of the part of the window inside the volume
template <typename I>
__global__ void __launch_bounds__(kThreads)
sw_acc_elem_k(const float* __restrict__ logits, int lld, float* __restrict__ acc, int ald, const float* __restrict__ td,
              const float* __restrict__ th, const float* __restrict__ tw, SwDims g, SwBox b) {
  const long total = (long)b.nz * b.ny * b.nx * g.C;
  const long li = (long)blockIdx.x * kThreads + threadIdx.x;
  if (li >= total) return;
  const I i = (I)li;
  const I v = i / (I)g.C;
  const int c = (int)(i - v * (I)g.C);
  const I r = v / (I)b.nx;
  const int x = b.x0 + (int)(v - r * (I)b.nx);
  const int zi = (int)(r / (I)b.ny);
  const int z = b.z0 + zi, y = b.y0 + (int)(r - (I)zi * (I)b.ny);
  const float w = rn_mul(rn_mul(td[z], th[y]), tw[x]);
  const long lo = ((((long)z * g.rh + y) * g.rw + x)) * lld + c;
  const long ao = ((((long)b.n * g.D + b.d0 + z) * g.H + b.h0 + y) * g.W + b.w0 + x) * ald + c;
  acc[ao] = rn_add(acc[ao], rn_mul(w, logits[lo]));
}

// ---- the passes of one window in one launch (msk_sw_accumulate_mirrored) ------------------------------------------------------
constexpr int kRunMax = 8;   // every subset of three axes

struct SwRun {      // by value in the kernel arguments: pass p reads src[p], mirrored about the window along the axes of mask[p]
  const float* src[kRunMax];
  int mask[kRunMax];
  int k;            // passes, 1 .. kRunMax, added in this order
  float scale;
};

// how the quad kernel reads a W-mirrored source row (the voxels are reversed, the channels inside a voxel are not)
enum { kWWhole = 0,    // C % 4 == 0: a quad lies inside one voxel, the mirrored voxel's quad is taken whole
       kWRev1 = 1,     // C == 1: the quad that ends where this one starts in the mirrored row, reversed
       kWSwap2 = 2,    // C == 2: the same quad, its two voxels swapped
       kWFloats = 3 }; // any other C: four 4-byte loads, a permutation inside the same cache lines

// the logits quad that pass (src, mask) adds to the accumulator quad at window-local (z, y), first float fx of the row
__device__ __forceinline__ float4 sw_mirrored_quad(const float* __restrict__ src, int mask, int z, int y, long fx, const SwDims& g, int wform) {
  const long rowlen = (long)g.rw * g.C;
  const float* row = src + ((long)(mask & 1 ? g.rd - 1 - z : z) * g.rh + (mask & 2 ? g.rh - 1 - y : y)) * rowlen;
  if (!(mask & 4)) return *reinterpret_cast<const float4*>(row + fx);
  if (wform == kWRev1 || wform == kWSwap2) {
    const float4 v = *reinterpret_cast<const float4*>(row + rowlen - 4 - fx);
    return wform == kWRev1 ? make_float4(v.w, v.z, v.y, v.x) : make_float4(v.z, v.w, v.x, v.y);
  }
  int x = (int)(fx / g.C), c = (int)(fx - (long)x * g.C);
  if (wform == kWWhole) return *reinterpret_cast<const float4*>(row + (long)(g.rw - 1 - x) * g.C + c);
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = row[(long)(g.rw - 1 - x) * g.C + c];
    if (++c == g.C) { c = 0; ++x; }
  }
  return make_float4(v[0], v[1], v[2], v[3]);
}

// sw_acc_quad_k for a run: the accumulator quad is loaded once, the run's passes are added in order, it is stored once
template <typename I>
__global__ void __launch_bounds__(kThreads)
sw_acc_run_quad_k(SwRun run, float* __restrict__ acc, const float* __restrict__ td, const float* __restrict__ th,
                  const float* __restrict__ tw, SwDims g, SwBox b, int wform) {
  const int rq = b.nx * g.C >> 2;
  const long total = (long)b.nz * b.ny * rq;
  const long li = (long)blockIdx.x * kThreads + threadIdx.x;
  if (li >= total) return;
  const I i = (I)li;
  const I r = i / (I)rq;
  const int q = (int)(i - r * (I)rq);
  const int zi = (int)(r / (I)b.ny);
  const int z = b.z0 + zi, y = b.y0 + (int)(r - (I)zi * (I)b.ny);
  const long fx = (long)b.x0 * g.C + 4L * q;
  const long ao = ((((long)b.n * g.D + b.d0 + z) * g.H + b.h0 + y) * g.W + b.w0) * g.C + fx;
  float4 l[kRunMax];
#pragma unroll
  for (int p = 0; p < kRunMax; ++p)                              // every load is issued before the first add
    if (p < run.k) l[p] = sw_mirrored_quad(run.src[p], run.mask[p], z, y, fx, g, wform);
  float4 a = *reinterpret_cast<const float4*>(acc + ao);
  const float wzy = rn_mul(td[z], th[y]);
  int xo = (4 * q) / g.C;                                        // voxel of the quad's first float, from x0
  int rem = 4 * q - xo * g.C;                                    // its channel
  const float* t = tw + b.x0;
  float w[4];
  w[0] = rn_mul(wzy, t[xo]);
#pragma unroll
  for (int j = 1; j < 4; ++j) {                                  // the quad's last float is inside the row: xo < nx
    w[j] = w[j - 1];
    if (++rem == g.C) { rem = 0; w[j] = rn_mul(wzy, t[++xo]); }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = rn_mul(w[j], run.scale);
#pragma unroll
  for (int p = 0; p < kRunMax; ++p)
    if (p < run.k) {
      a.x = rn_add(a.x, rn_mul(w[0], l[p].x));
      a.y = rn_add(a.y, rn_mul(w[1], l[p].y));
      a.z = rn_add(a.z, rn_mul(w[2], l[p].z));
      a.w = rn_add(a.w, rn_mul(w[3], l[p].w));
    }
  *reinterpret_cast<float4*>(acc + ao) = a;
}

// sw_acc_elem_k for a run
template <typename I>
__global__ void __launch_bounds__(kThreads)
sw_acc_run_elem_k(SwRun run, int lld, float* __restrict__ acc, int ald, const float* __restrict__ td, const float* __restrict__ th,
                  const float* __restrict__ tw, SwDims g, SwBox b) {
  const long total = (long)b.nz * b.ny * b.nx * g.C;
  const long li = (long)blockIdx.x * kThreads + threadIdx.x;
  if (li >= total) return;
  const I i = (I)li;
  const I v = i / (I)g.C;
  const int c = (int)(i - v * (I)g.C);
  const I r = v / (I)b.nx;
  const int x = b.x0 + (int)(v - r * (I)b.nx);
  const int zi = (int)(r / (I)b.ny);
  const int z = b.z0 + zi, y = b.y0 + (int)(r - (I)zi * (I)b.ny);
  const float w = rn_mul(rn_mul(rn_mul(td[z], th[y]), tw[x]), run.scale);
  const long ao = ((((long)b.n * g.D + b.d0 + z) * g.H + b.h0 + y) * g.W + b.w0 + x) * ald + c;
  float l[kRunMax];
#pragma unroll
  for (int p = 0; p < kRunMax; ++p)
    if (p < run.k) {
      const int m = run.mask[p];
      const int mz = m & 1 ? g.rd - 1 - z : z, my = m & 2 ? g.rh - 1 - y : y, mx = m & 4 ? g.rw - 1 - x : x;
      l[p] = run.src[p][(((long)mz * g.rh + my) * g.rw + mx) * lld + c];
    }
  float a = acc[ao];
#pragma unroll
  for (int p = 0; p < kRunMax; ++p)
    if (p < run.k) a = rn_add(a, rn_mul(w, l[p]));
  acc[ao] = a;
}

inline bool disjoint(const msk_tensor& a, const msk_tensor& b) {
  const uintptr_t a0 = (uintptr_t)a.p, a1 = a0 + ((size_t)(msk_voxels(a) - 1) * a.ld + a.c) * sizeof(float);
  const uintptr_t b0 = (uintptr_t)b.p, b1 = b0 + ((size_t)(msk_voxels(b) - 1) * b.ld + b.c) * sizeof(float);
  return a1 <= b0 || b1 <= a0;
}
// the part [first, first + count) of a window axis of extent r at origin o that lies inside [0, size); false: none
inline bool clip_axis(int o, int r, int size, int* first, int* count) {
  const long lo = o < 0 ? -(long)o : 0, hi = (long)o + r > size ? (long)size - o : r;
  if (hi <= lo) return false;
  *first = (int)lo;
  *count = (int)(hi - lo);
  return true;
}
inline bool clip_box(const msk_tensor& vol, const msk_tensor& win, const int32_t* o, SwBox* b) {
  b->n = o[0]; b->d0 = o[1]; b->h0 = o[2]; b->w0 = o[3];
  return clip_axis(o[1], win.d, vol.d, &b->z0, &b->nz) && clip_axis(o[2], win.h, vol.h, &b->y0, &b->ny) &&
         clip_axis(o[3], win.w, vol.w, &b->x0, &b->nx);
}
inline SwDims dims_of(const msk_tensor& vol, const msk_tensor& win) {
  SwDims g;
  g.D = vol.d; g.H = vol.h; g.W = vol.w;
  g.rd = win.d; g.rh = win.h; g.rw = win.w;
  g.C = win.c;
  return g;
}
inline long blocks_for(long total) { return (total + kThreads - 1) / kThreads; }

// the per-thread index arithmetic (two or three divisions) in 32 bits where the window's element count allows it
#define SW_LAUNCH(kernel, total, ...)                                                                                      \
  do {                                                                                                                     \
    if ((total) <= (long)UINT_MAX)                                                                                         \
      hipLaunchKernelGGL(kernel<unsigned>, dim3((unsigned)blocks_for(total)), dim3(kThreads), 0, ctx->stream, __VA_ARGS__); \
    else                                                                                                                   \
      hipLaunchKernelGGL(kernel<long>, dim3((unsigned)blocks_for(total)), dim3(kThreads), 0, ctx->stream, __VA_ARGS__);     \
  } while (0)

// msk_sw_gather (cols = 4, no mirror) and msk_sw_gather_mirrored (cols = 5, the fifth int of a row is its mask)
int gather(msk_ctx* ctx, const msk_tensor& vol, const msk_tensor& patches, const int32_t* origins, int cols, float cval, const char* tag) {
  MSK_REQUIRE(ctx, msk_well_formed(vol) && msk_well_formed(patches), "vol/patches must be non-empty float tensors with ld >= c");
  MSK_REQUIRE(ctx, vol.c == patches.c, "vol/patches channel mismatch");
  MSK_REQUIRE(ctx, origins != nullptr, "origins must be a host array of patches.n x 4 (mirrored: 5) int32");
  MSK_REQUIRE(ctx, disjoint(vol, patches), "patches must not overlap vol");
  const SwDims g = dims_of(vol, patches);
  // the quad kernel stores whole patch quads and indexes the volume as dense (ld == c): a channel-slice view on either side takes
  // the element kernel, and so does a W mirror of more than one channel (the voxels are reversed, their channels are not)
  const bool quads = msk_quad_dense(patches) && vol.ld == vol.c && ((long)g.rw * g.C) % 4 == 0;
  const long efloats = (long)g.rd * g.rh * g.rw * g.C, equads = (long)g.rd * g.rh * (g.rw * (long)g.C / 4);
  MSK_REQUIRE(ctx, blocks_for(quads && cols == 4 ? equads : efloats) <= INT_MAX, "window too large");
  SwBox b;
  for (int k = 0; k < patches.n; ++k) {
    const int32_t* o = origins + cols * k;
    MSK_REQUIRE(ctx, o[0] >= 0 && o[0] < vol.n, "origins: n outside the batch of vol");
    MSK_REQUIRE(ctx, clip_box(vol, patches, o, &b), "origins: a window does not intersect the volume");
    MSK_REQUIRE(ctx, cols == 4 || (o[4] >= 0 && o[4] <= 7), "origins: mask outside 0..7");
  }
  msk_launch_scope ls(ctx, tag);
  const long wfloats = (long)g.rd * g.rh * g.rw * patches.ld;   // floats between two windows of patches
  for (int k = 0; k < patches.n; ++k) {
    const int32_t* o = origins + cols * k;
    const int mask = cols == 4 ? 0 : o[4];
    clip_box(vol, patches, o, &b);
    float* dst = (float*)patches.p + k * wfloats;
    if (quads && (!(mask & 4) || g.C == 1)) {
      // whole source quads: dense volume whose rows and this window's row start are whole quads
      const int src_quads = msk_quad_dense(vol) && ((long)g.W * g.C) % 4 == 0 && ((long)b.w0 * g.C) % 4 == 0;
      SW_LAUNCH(sw_gather_quad_k, equads, (const float*)vol.p, dst, g, b, cval, src_quads, mask);
    } else {
      SW_LAUNCH(sw_gather_elem_k, efloats, (const float*)vol.p, vol.ld, dst, patches.ld, g, b, cval, mask);
    }
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // namespace

extern "C" {

int msk_sw_gather(msk_ctx* ctx, msk_tensor vol, msk_tensor patches, const int32_t* origins, float cval) {
  return gather(ctx, vol, patches, origins, 4, cval, "sw_gather");
}

int msk_sw_gather_mirrored(msk_ctx* ctx, msk_tensor vol, msk_tensor patches, const int32_t* origins, float cval) {
  return gather(ctx, vol, patches, origins, 5, cval, "sw_gather_mirrored");
}

int msk_sw_accumulate(msk_ctx* ctx, msk_tensor logits, const int32_t* origins, const float* td, int nd, const float* th, int nh,
                      const float* tw, int nw, msk_tensor acc) {
  MSK_REQUIRE(ctx, msk_well_formed(logits) && msk_well_formed(acc), "logits/acc must be non-empty float tensors with ld >= c");
  MSK_REQUIRE(ctx, logits.c == acc.c, "logits/acc channel mismatch");
  MSK_REQUIRE(ctx, origins != nullptr, "origins must be a host array of logits.n x 7 int32");
  MSK_REQUIRE(ctx, td != nullptr && th != nullptr && tw != nullptr && ((((uintptr_t)td) | ((uintptr_t)th) | ((uintptr_t)tw)) & 3) == 0,
              "td/th/tw must be 4-byte aligned device tables");
  MSK_REQUIRE(ctx, nd >= 1 && nh >= 1 && nw >= 1, "td/th/tw need at least one row each");
  MSK_REQUIRE(ctx, disjoint(logits, acc), "acc must not overlap the logits");
  const SwDims g = dims_of(acc, logits);
  MSK_REQUIRE(ctx, blocks_for((long)g.rd * g.rh * g.rw * g.C) <= INT_MAX, "window too large");
  SwBox b;
  for (int k = 0; k < logits.n; ++k) {
    const int32_t* o = origins + 7 * k;
    MSK_REQUIRE(ctx, o[0] >= 0 && o[0] < acc.n, "origins: n outside the batch of acc");
    MSK_REQUIRE(ctx, o[4] >= 0 && o[4] < nd && o[5] >= 0 && o[5] < nh && o[6] >= 0 && o[6] < nw, "origins: table row outside its table");
    MSK_REQUIRE(ctx, clip_box(acc, logits, o, &b), "origins: a window does not intersect the volume");
  }
  msk_launch_scope ls(ctx, "sw_accumulate");
  const bool dense = msk_quad_dense(logits) && msk_quad_dense(acc) && ((long)g.rw * g.C) % 4 == 0 && ((long)g.W * g.C) % 4 == 0;
  const long wfloats = (long)g.rd * g.rh * g.rw * logits.ld;
  for (int k = 0; k < logits.n; ++k) {
    const int32_t* o = origins + 7 * k;
    clip_box(acc, logits, o, &b);
    const float* src = (const float*)logits.p + k * wfloats;
    const float* rd_ = td + (long)o[4] * g.rd;
    const float* rh_ = th + (long)o[5] * g.rh;
    const float* rw_ = tw + (long)o[6] * g.rw;
    // row starts in both tensors and the row length are whole quads
    if (dense && ((long)b.x0 * g.C) % 4 == 0 && (((long)b.w0 + b.x0) * g.C) % 4 == 0 && ((long)b.nx * g.C) % 4 == 0) {
      const long total = (long)b.nz * b.ny * (b.nx * (long)g.C / 4);
      SW_LAUNCH(sw_acc_quad_k, total, src, (float*)acc.p, rd_, rh_, rw_, g, b);
    } else {
      const long total = (long)b.nz * b.ny * b.nx * g.C;
      SW_LAUNCH(sw_acc_elem_k, total, src, logits.ld, (float*)acc.p, acc.ld, rd_, rh_, rw_, g, b);
    }
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

int msk_sw_accumulate_mirrored(msk_ctx* ctx, msk_tensor logits, const int32_t* origins, const float* td, int nd, const float* th,
                               int nh, const float* tw, int nw, float scale, msk_tensor acc) {
  MSK_REQUIRE(ctx, msk_well_formed(logits) && msk_well_formed(acc), "logits/acc must be non-empty float tensors with ld >= c");
  MSK_REQUIRE(ctx, logits.c == acc.c, "logits/acc channel mismatch");
  MSK_REQUIRE(ctx, origins != nullptr, "origins must be a host array of logits.n x 8 int32");
  MSK_REQUIRE(ctx, td != nullptr && th != nullptr && tw != nullptr && ((((uintptr_t)td) | ((uintptr_t)th) | ((uintptr_t)tw)) & 3) == 0,
              "td/th/tw must be 4-byte aligned device tables");
  MSK_REQUIRE(ctx, nd >= 1 && nh >= 1 && nw >= 1, "td/th/tw need at least one row each");
  MSK_REQUIRE(ctx, std::isfinite(scale) && scale > 0.f, "scale must be finite and positive");
  MSK_REQUIRE(ctx, disjoint(logits, acc), "acc must not overlap the logits");
  const SwDims g = dims_of(acc, logits);
  MSK_REQUIRE(ctx, blocks_for((long)g.rd * g.rh * g.rw * g.C) <= INT_MAX, "window too large");
  SwBox b;
  for (int k = 0; k < logits.n; ++k) {
    const int32_t* o = origins + 8 * k;
    MSK_REQUIRE(ctx, o[0] >= 0 && o[0] < acc.n, "origins: n outside the batch of acc");
    MSK_REQUIRE(ctx, o[4] >= 0 && o[4] < nd && o[5] >= 0 && o[5] < nh && o[6] >= 0 && o[6] < nw, "origins: table row outside its table");
    MSK_REQUIRE(ctx, clip_box(acc, logits, o, &b), "origins: a window does not intersect the volume");
    MSK_REQUIRE(ctx, o[7] >= 0 && o[7] <= 7, "origins: mask outside 0..7");
  }
  msk_launch_scope ls(ctx, "sw_accumulate_mirrored");
  const bool dense = msk_quad_dense(logits) && msk_quad_dense(acc) && ((long)g.rw * g.C) % 4 == 0 && ((long)g.W * g.C) % 4 == 0;
  const int wform = g.C % 4 == 0 ? kWWhole : g.C == 1 ? kWRev1 : g.C == 2 ? kWSwap2 : kWFloats;
  const long wfloats = (long)g.rd * g.rh * g.rw * logits.ld;
  for (int k = 0; k < logits.n;) {
    const int32_t* o = origins + 8 * k;
    SwRun run;                                                  // the rows of this window that follow each other, 8 at the most
    run.scale = scale;
    run.k = 0;
    while (run.k < kRunMax && k + run.k < logits.n && memcmp(o, o + 8 * run.k, 7 * sizeof(int32_t)) == 0) {
      run.src[run.k] = (const float*)logits.p + (k + run.k) * wfloats;
      run.mask[run.k] = o[8 * run.k + 7];
      ++run.k;
    }
    for (int p = run.k; p < kRunMax; ++p) { run.src[p] = nullptr; run.mask[p] = 0; }   // never read
    clip_box(acc, logits, o, &b);
    const float* rd_ = td + (long)o[4] * g.rd;
    const float* rh_ = th + (long)o[5] * g.rh;
    const float* rw_ = tw + (long)o[6] * g.rw;
    // row starts in both tensors and the row length are whole quads
    if (dense && ((long)b.x0 * g.C) % 4 == 0 && (((long)b.w0 + b.x0) * g.C) % 4 == 0 && ((long)b.nx * g.C) % 4 == 0) {
      const long total = (long)b.nz * b.ny * (b.nx * (long)g.C / 4);
      SW_LAUNCH(sw_acc_run_quad_k, total, run, (float*)acc.p, rd_, rh_, rw_, g, b, wform);
    } else {
      const long total = (long)b.nz * b.ny * b.nx * g.C;
      SW_LAUNCH(sw_acc_run_elem_k, total, run, logits.ld, (float*)acc.p, acc.ld, rd_, rh_, rw_, g, b);
    }
    k += run.k;
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
