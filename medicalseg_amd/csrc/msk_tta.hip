// Test-time augmentation (core/infer.py aug_inference): mirror an NDHWC tensor along any subset of D/H/W in one pass, fold
// "softmax over C of the mirrored logits, added to the running sum" into one read and one read-modify-write, and finish with
// the mean and the argmax.  Every float operation is spelled with __fadd_rn / __fmul_rn where a multiply feeds an add: the
// results are pinned bit for bit against msk_softmax_c + numpy float32 (tests/tta_reference.py), an FMA would differ.
//
// Thread-to-element map of the tile kernels (dense tensors whose W rows are whole 16-byte quads): a workgroup owns R whole W
// rows of the output (or one chunk of a long row).  Mirroring D / H moves whole rows, mirroring W reverses the voxels INSIDE a
// row, so the source of every output row (chunk) is one contiguous run: it is loaded in source order with 16 bytes per lane
// (1 KiB per wavefront instruction, whatever C is), the W mirror happens between two LDS images with one thread per voxel, and
// the output leaves in output order with 16 bytes per lane again.  A thread-per-voxel kernel on global memory moves 4*C bytes
// per lane at a stride of 4*C (12 bytes at C = 3, 80 at C = 20); that form remains as the path of channel-slice views
// (ld > c), rows that are no whole quads, and very large C.
#include "msk_common.h"

#include <climits>

namespace {

constexpr int kThreads = 256;
constexpr int kTileFloats = 7680;   // floats of one LDS image of a tile: two images + the row table stay under 64 KiB
constexpr int kMinTileVoxels = 32;  // fewer voxels per tile than this (C > 240): the direct kernels

struct TtaGeom {
  int D, H, W, C;
  long rows;      // N * D * H
  int R;          // rows per tile
  int Wt;         // voxels of a row per tile (W, or a multiple of 4 below it)
  int wchunks;    // ceil(W / Wt)
  int mask;       // bit 0 = D, bit 1 = H, bit 2 = W
  int img;        // floats between the two LDS images (0: the W axis is not mirrored, one image in place)
};

// flat row index (n, d, h) -> the row it is read from
__device__ __forceinline__ long tta_src_row(long r, int D, int H, int mask) {
  const long t = r / H;
  int h = (int)(r - t * H);
  const long n = t / D;
  int d = (int)(t - n * D);
  if (mask & 1) d = D - 1 - d;
  if (mask & 2) h = H - 1 - h;
  return (n * D + d) * H + h;
}

// The arithmetic of softmax_c_k (msk_elementwise.hip) on one voxel: running fmaxf, s += expf(x - m) in channel order,
// inv = 1 / s, p = expf(x - m) * inv.  o may be x.
__device__ __forceinline__ void tta_softmax(const float* x, float* o, int C) {
  float m = x[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
  float s = 0.f;
  for (int c = 0; c < C; ++c) {
    const float e = expf(x[c] - m);
    o[c] = e;
    s = __fadd_rn(s, e);
  }
  const float inv = 1.f / s;
  for (int c = 0; c < C; ++c) o[c] = __fmul_rn(o[c], inv);
}

// SOFTMAX = false: dst = mirror(src).  SOFTMAX = true: dst = first ? p : dst + p with p = softmax_c(mirror(src)).
template <bool SOFTMAX>
__global__ void __launch_bounds__(kThreads)
tta_tile_k(const float* __restrict__ src, float* __restrict__ dst, TtaGeom g, int first) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  long* srow = reinterpret_cast<long*>(smem);                      // kThreads entries
  float4* in4 = reinterpret_cast<float4*>(smem + kThreads * sizeof(long));
  float* in = reinterpret_cast<float*>(in4);
  float* out = in + g.img;
  const float4* out4 = reinterpret_cast<const float4*>(out);

  const long rg = blockIdx.x / g.wchunks;
  const int wc = (int)(blockIdx.x - rg * g.wchunks);
  const long r0 = rg * g.R;
  const int nr = (int)(g.rows - r0 < g.R ? g.rows - r0 : g.R);
  const int w0 = wc * g.Wt;
  const int wt = g.W - w0 < g.Wt ? g.W - w0 : g.Wt;
  const int ws0 = (g.mask & 4) ? g.W - w0 - wt : w0;               // first source voxel of the chunk
  if ((int)threadIdx.x < nr) srow[threadIdx.x] = tta_src_row(r0 + threadIdx.x, g.D, g.H, g.mask);
  __syncthreads();

  const int rq = wt * g.C >> 2;                                    // quads of one row chunk
  const int nq = nr * rq;
  const float4* s4 = reinterpret_cast<const float4*>(src);
  for (int i = threadIdx.x; i < nq; i += kThreads) {
    const int r = i / rq, q = i - r * rq;
    in4[i] = s4[(((srow[r] * g.W + ws0) * g.C) >> 2) + q];
  }
  __syncthreads();

  if ((int)threadIdx.x < nr * wt) {                                // one voxel per thread
    const int r = threadIdx.x / wt, wl = threadIdx.x - r * wt;
    const int wsl = (g.mask & 4) ? wt - 1 - wl : wl;
    const float* x = in + (long)(r * wt + wsl) * g.C;
    float* o = out + (long)(r * wt + wl) * g.C;
    if (SOFTMAX) {
      tta_softmax(x, o, g.C);
    } else if (g.img) {
      for (int c = 0; c < g.C; ++c) o[c] = x[c];
    }
  }
  __syncthreads();

  float4* d4 = reinterpret_cast<float4*>(dst);
  for (int i = threadIdx.x; i < nq; i += kThreads) {
    const int r = i / rq, q = i - r * rq;
    const long di = ((((r0 + r) * g.W + w0) * g.C) >> 2) + q;
    float4 p = out4[i];
    if (SOFTMAX && !first) {
      const float4 a = d4[di];
      p.x = __fadd_rn(a.x, p.x); p.y = __fadd_rn(a.y, p.y); p.z = __fadd_rn(a.z, p.z); p.w = __fadd_rn(a.w, p.w);
    }
    d4[di] = p;
  }
}

// any ld, any extents: one thread per element
__global__ void __launch_bounds__(kThreads)
flip_direct_k(const float* __restrict__ src, int sld, float* __restrict__ dst, int dld, long total, int D, int H, int W, int C,
              int mask) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long v = i / C;
    const int c = (int)(i - v * C);
    const long r = v / W;
    int w = (int)(v - r * W);
    if (mask & 4) w = W - 1 - w;
    dst[v * dld + c] = src[(tta_src_row(r, D, H, mask) * W + w) * sld + c];
  }
}

// any ld, any extents: one thread per voxel (consecutive lanes read consecutive voxels, reversed under a W mirror)
__global__ void __launch_bounds__(kThreads)
tta_acc_direct_k(const float* __restrict__ x, int xld, float* __restrict__ acc, int ald, long voxels, int D, int H, int W, int C,
                 int mask, int first) {
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < voxels; v += (long)gridDim.x * blockDim.x) {
    const long r = v / W;
    int w = (int)(v - r * W);
    if (mask & 4) w = W - 1 - w;
    const float* p = x + (tta_src_row(r, D, H, mask) * W + w) * xld;
    float m = p[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, p[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s = __fadd_rn(s, expf(p[c] - m));
    const float inv = 1.f / s;
    float* a = acc + v * ald;
    for (int c = 0; c < C; ++c) {
      const float q = __fmul_rn(expf(p[c] - m), inv);
      a[c] = first ? q : __fadd_rn(a[c], q);
    }
  }
}

// probs = acc * r, pred = argmax over c of acc (first maximum wins, argmax_k).  Tiles of TV consecutive voxels: acc streams
// through with 16 bytes per lane, the mean leaves the same way, the argmax reads the tile's LDS image.
__global__ void __launch_bounds__(kThreads)
tta_finish_tile_k(const float* __restrict__ acc, long voxels, int C, int TV, float r, float* __restrict__ probs,
                  int32_t* __restrict__ pred) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* t4 = reinterpret_cast<float4*>(smem);
  float* t = reinterpret_cast<float*>(smem);
  const long v0 = (long)blockIdx.x * TV;
  const int nv = (int)(voxels - v0 < TV ? voxels - v0 : TV);
  const int nf = nv * C, nq = nf >> 2;
  const long f0 = v0 * C;                                          // a multiple of 4: TV is
  const float4* a4 = reinterpret_cast<const float4*>(acc + f0);
  float4* p4 = reinterpret_cast<float4*>(probs + f0);
  for (int i = threadIdx.x; i < nq; i += kThreads) {
    const float4 a = a4[i];
    if (pred) t4[i] = a;
    if (probs) p4[i] = make_float4(__fmul_rn(a.x, r), __fmul_rn(a.y, r), __fmul_rn(a.z, r), __fmul_rn(a.w, r));
  }
  for (int i = (nq << 2) + threadIdx.x; i < nf; i += kThreads) {   // the last tile's odd floats
    const float a = acc[f0 + i];
    if (pred) t[i] = a;
    if (probs) probs[f0 + i] = __fmul_rn(a, r);
  }
  if (!pred) return;
  __syncthreads();
  if ((int)threadIdx.x < nv) {
    const float* p = t + threadIdx.x * C;
    float best = p[0];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
      const float q = p[c];
      if (q > best) {
        best = q;
        bi = c;
      }
    }
    pred[v0 + threadIdx.x] = bi;
  }
}

__global__ void __launch_bounds__(kThreads)
tta_finish_direct_k(const float* __restrict__ acc, int ald, long voxels, int C, float r, float* __restrict__ probs, int pld,
                    int32_t* __restrict__ pred) {
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < voxels; v += (long)gridDim.x * blockDim.x) {
    const float* p = acc + v * ald;
    float best = p[0];
    int bi = 0;
    for (int c = 0; c < C; ++c) {
      const float q = p[c];
      if (q > best) {
        best = q;
        bi = c;
      }
      if (probs) probs[v * pld + c] = __fmul_rn(q, r);
    }
    if (pred) pred[v] = bi;
  }
}

// tile geometry of tta_tile_k; false: the tensors need the direct kernels
bool tile_geom(const msk_tensor& src, const msk_tensor& dst, int mask, TtaGeom* g) {
  if (!msk_quad_dense(src) || !msk_quad_dense(dst) || ((long)src.w * src.c) % 4 != 0) return false;
  int tv = kTileFloats / src.c;
  if (tv > kThreads) tv = kThreads;
  if (tv < kMinTileVoxels) return false;
  g->D = src.d; g->H = src.h; g->W = src.w; g->C = src.c;
  g->rows = (long)src.n * src.d * src.h;
  if (src.w <= tv) {
    g->R = tv / src.w;
    g->Wt = src.w;
  } else {
    g->R = 1;
    g->Wt = tv & ~3;   // chunk starts on a quad whatever C is
  }
  g->wchunks = (src.w + g->Wt - 1) / g->Wt;
  g->mask = mask;
  g->img = (mask & 4) ? g->R * g->Wt * src.c : 0;
  const long tiles = ((g->rows + g->R - 1) / g->R) * g->wchunks;
  return tiles <= INT_MAX;
}
inline size_t tile_lds(const TtaGeom& g) {
  return kThreads * sizeof(long) + (size_t)(g.img ? 2 : 1) * g.R * g.Wt * g.C * sizeof(float);
}
inline unsigned tile_count(const TtaGeom& g) { return (unsigned)(((g.rows + g.R - 1) / g.R) * g.wchunks); }

}  // namespace

extern "C" {

int msk_flip_axes(msk_ctx* ctx, msk_tensor src, msk_tensor dst, int mask) {
  MSK_REQUIRE(ctx, msk_well_formed(src) && msk_well_formed(dst), "src/dst must be non-empty float tensors with ld >= c");
  MSK_REQUIRE(ctx, msk_same_shape(src, dst), "src/dst shape mismatch");
  MSK_REQUIRE(ctx, mask >= 0 && mask <= 7, "mask must be in 0..7 (bit 0 = D, bit 1 = H, bit 2 = W)");
  MSK_REQUIRE(ctx, src.p != dst.p, "msk_flip_axes is out of place");
  TtaGeom g;
  msk_launch_scope ls(ctx, "flip_axes");
  if (tile_geom(src, dst, mask, &g)) {
    hipLaunchKernelGGL(tta_tile_k<false>, dim3(tile_count(g)), dim3(kThreads), tile_lds(g), ctx->stream, (const float*)src.p,
                       (float*)dst.p, g, 0);
  } else {
    const long total = msk_voxels(src) * src.c;
    hipLaunchKernelGGL(flip_direct_k, dim3(msk_ew_blocks(total, ctx->num_cu)), dim3(kThreads), 0, ctx->stream,
                       (const float*)src.p, src.ld, (float*)dst.p, dst.ld, total, src.d, src.h, src.w, src.c, mask);
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

int msk_tta_accumulate(msk_ctx* ctx, msk_tensor logits, int mask, msk_tensor acc, int first) {
  MSK_REQUIRE(ctx, msk_well_formed(logits) && msk_well_formed(acc), "logits/acc must be non-empty float tensors with ld >= c");
  MSK_REQUIRE(ctx, msk_same_shape(logits, acc), "logits/acc shape mismatch");
  MSK_REQUIRE(ctx, mask >= 0 && mask <= 7, "mask must be in 0..7 (bit 0 = D, bit 1 = H, bit 2 = W)");
  MSK_REQUIRE(ctx, logits.p != acc.p, "acc must not be the logits");
  TtaGeom g;
  msk_launch_scope ls(ctx, "tta_accumulate");
  if (tile_geom(logits, acc, mask, &g)) {
    hipLaunchKernelGGL(tta_tile_k<true>, dim3(tile_count(g)), dim3(kThreads), tile_lds(g), ctx->stream, (const float*)logits.p,
                       (float*)acc.p, g, first ? 1 : 0);
  } else {
    const long voxels = msk_voxels(logits);
    hipLaunchKernelGGL(tta_acc_direct_k, dim3(msk_ew_blocks(voxels, ctx->num_cu)), dim3(kThreads), 0, ctx->stream,
                       (const float*)logits.p, logits.ld, (float*)acc.p, acc.ld, voxels, logits.d, logits.h, logits.w, logits.c,
                       mask, first ? 1 : 0);
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

int msk_tta_finish(msk_ctx* ctx, msk_tensor acc, int passes, msk_tensor probs, int32_t* pred) {
  MSK_REQUIRE(ctx, msk_well_formed(acc), "acc must be a non-empty float tensor with ld >= c");
  MSK_REQUIRE(ctx, passes >= 1, "passes must be >= 1");
  MSK_REQUIRE(ctx, probs.p == nullptr || (msk_well_formed(probs) && msk_same_shape(acc, probs)), "acc/probs shape mismatch");
  MSK_REQUIRE(ctx, (((uintptr_t)pred) & 3) == 0, "pred must be a 4-byte aligned device pointer");
  if (probs.p == nullptr && pred == nullptr) return 0;
  const float r = 1.f / (float)passes;
  const long voxels = msk_voxels(acc);
  int tv = kTileFloats / acc.c;
  if (tv > kThreads) tv = kThreads;
  tv &= ~3;
  const long tiles = tv > 0 ? (voxels + tv - 1) / tv : 0;
  msk_launch_scope ls(ctx, "tta_finish");
  if (msk_quad_dense(acc) && (probs.p == nullptr || msk_quad_dense(probs)) && tv >= kMinTileVoxels && tiles <= INT_MAX) {
    hipLaunchKernelGGL(tta_finish_tile_k, dim3((unsigned)tiles), dim3(kThreads), (size_t)tv * acc.c * sizeof(float), ctx->stream,
                       (const float*)acc.p, voxels, acc.c, tv, r, (float*)probs.p, pred);
  } else {
    hipLaunchKernelGGL(tta_finish_direct_k, dim3(msk_ew_blocks(voxels, ctx->num_cu)), dim3(kThreads), 0, ctx->stream,
                       (const float*)acc.p, acc.ld, voxels, acc.c, r, (float*)probs.p, probs.p ? probs.ld : 0, pred);
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
