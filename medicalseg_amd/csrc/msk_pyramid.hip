// Label pyramid of nnU-Net's deep supervision (models/losses/fused.py label_pyramid): the int32 label [N, D, H, W] down-sampled by
// nearest neighbour to up to 8 extents in one launch, per axis i = ((2 o + 1) * in) / (2 * out) in integers
// (tests/pyramid_reference.py).
//
// Thread-to-element map: a thread owns four consecutive output voxels of one W row (a "quad"; the last quad of a row whose
// extent is no multiple of 4 is partial), consecutive lanes own consecutive quads, so where ow % 4 == 0 and the level's
// destination is 16-byte aligned a wavefront stores 1 KiB contiguously with 16 bytes per lane; any other level stores 4 bytes
// per voxel.  That choice is per level, hence per workgroup.  The four sources of a quad lie in one source row at the stride
// in / out; all four loads are issued before the store form is chosen (a voxel past the end of a partial quad reads the row's
// last source and is not stored).  In the ISA: four global_load_dword ahead of the first s_waitcnt, then one global_store_dwordx4,
// or up to four global_store_dword; the quad is stored as ONE native vector value because a struct of four ints is four IR
// stores, of which the optimiser moved the last one into the code shared with the 4-byte form (leaving dwordx3 + dword and the
// fourth load behind a wait).  18 VGPRs, no scratch.  Workgroups are dealt to the levels in order: level l owns the
// workgroups [first_l, first_l + ceil(quads_l / 256)), and a workgroup finds its level by walking the (at most 8) first-block
// offsets, which travel with the extents and the destination pointers by value in the kernel arguments.  The launch is
// launch-bound at every shape the package uses (the three levels of a 512 x 512 x 12 label are 2.95 MB): no LDS, no atomics,
// no grid-stride loop, nothing for the host to read.
#include "msk_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLevels = 8;
constexpr int kMaxAxis = 32768;   // (2 o + 1) * in < 2 * in * in <= 2^31: the index products stay inside 32 bits

struct PyrLevel {
  int32_t* dst;
  int od, oh, ow;
  int qpr;          // quads per output row: ceil(ow / 4)
  unsigned quads;   // N * od * oh * qpr
  unsigned first;   // first workgroup of this level
  int vec;          // ow % 4 == 0 and dst 16-byte aligned: one 16-byte store per quad
};

struct PyrTable {
  PyrLevel lv[kMaxLevels];
  int levels;
  int D, H, W;
};

typedef int32_t pyr_quad __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int pyr_src(int o, int in, int out) { return ((2 * o + 1) * in) / (2 * out); }

__global__ void __launch_bounds__(kThreads)
label_pyramid_k(const int32_t* __restrict__ src, PyrTable t) {
  int l = 0;
  for (int i = 1; i < t.levels; ++i)
    if (blockIdx.x >= t.lv[i].first) l = i;
  const PyrLevel& L = t.lv[l];
  const unsigned q = (blockIdx.x - L.first) * kThreads + threadIdx.x;
  if (q >= L.quads) return;
  const unsigned row = q / (unsigned)L.qpr;                 // (n, z, y) flat
  const int x0 = (int)(q - row * (unsigned)L.qpr) * 4;
  const unsigned nz = row / (unsigned)L.oh;
  const int y = (int)(row - nz * (unsigned)L.oh);
  const unsigned n = nz / (unsigned)L.od;
  const int z = (int)(nz - n * (unsigned)L.od);
  const int32_t* srow = src + ((n * (unsigned)t.D + (unsigned)pyr_src(z, t.D, L.od)) * (unsigned)t.H +
                               (unsigned)pyr_src(y, t.H, L.oh)) * (unsigned)t.W;
  int32_t* drow = L.dst + row * (unsigned)L.ow + (unsigned)x0;
  // all four loads go out before the (workgroup-uniform) choice of the store form: a voxel past the end of the row reads the
  // row's last source instead (a valid address) and is not stored
  const int last = L.ow - 1;
  int4 v;
  v.x = srow[pyr_src(x0, t.W, L.ow)];
  v.y = srow[pyr_src(min(x0 + 1, last), t.W, L.ow)];
  v.z = srow[pyr_src(min(x0 + 2, last), t.W, L.ow)];
  v.w = srow[pyr_src(min(x0 + 3, last), t.W, L.ow)];
  if (L.vec) {
    *reinterpret_cast<pyr_quad*>(drow) = pyr_quad{v.x, v.y, v.z, v.w};   // one vector value: not four stores the optimiser may share out
  } else {
    drow[0] = v.x;
    if (x0 + 1 <= last) drow[1] = v.y;
    if (x0 + 2 <= last) drow[2] = v.z;
    if (x0 + 3 <= last) drow[3] = v.w;
  }
}

}  // namespace

extern "C" {

int msk_label_pyramid(msk_ctx* ctx, const int32_t* label, int n, int d, int h, int w, int levels, const int32_t* extents,
                      int32_t* const* dst) {
  MSK_REQUIRE(ctx, label != nullptr && extents != nullptr && dst != nullptr, "label, extents and dst must not be null");
  MSK_REQUIRE(ctx, (((uintptr_t)label) & 3) == 0, "label must be a 4-byte aligned device pointer");
  MSK_REQUIRE(ctx, levels >= 1 && levels <= kMaxLevels, "levels must be in 1..8");
  MSK_REQUIRE(ctx, n >= 1 && d >= 1 && h >= 1 && w >= 1, "the label must not be empty");
  MSK_REQUIRE(ctx, d <= kMaxAxis && h <= kMaxAxis && w <= kMaxAxis, "an axis of the label is longer than 32768");
  const long plane = (long)d * h * w;                       // <= 2^45
  MSK_REQUIRE(ctx, n <= ((1L << 31) - 1) / plane, "the label has 2^31 voxels or more");   // no product that could overflow
  const long total = n * plane;
  const uintptr_t s0 = (uintptr_t)label, s1 = s0 + (uintptr_t)total * 4;
  PyrTable t;
  memset(&t, 0, sizeof(t));
  t.levels = levels;
  t.D = d; t.H = h; t.W = w;
  unsigned blocks = 0;
  for (int l = 0; l < levels; ++l) {
    const int od = extents[3 * l], oh = extents[3 * l + 1], ow = extents[3 * l + 2];
    MSK_REQUIRE(ctx, od >= 1 && od <= d && oh >= 1 && oh <= h && ow >= 1 && ow <= w,
                "every extent of a level must be in 1..the label's extent of that axis");
    MSK_REQUIRE(ctx, dst[l] != nullptr && (((uintptr_t)dst[l]) & 3) == 0, "dst[l] must be a 4-byte aligned device pointer");
    const long out = (long)n * od * oh * ow;                // <= total < 2^31
    const uintptr_t d0 = (uintptr_t)dst[l], d1 = d0 + (uintptr_t)out * 4;
    MSK_REQUIRE(ctx, d1 <= s0 || d0 >= s1, "a destination overlaps the label");
    PyrLevel& L = t.lv[l];
    L.dst = dst[l];
    L.od = od; L.oh = oh; L.ow = ow;
    L.qpr = (ow + 3) / 4;
    L.quads = (unsigned)((long)n * od * oh * L.qpr);        // <= out
    L.first = blocks;
    L.vec = (ow % 4 == 0 && (d0 & 15) == 0) ? 1 : 0;
    blocks += (L.quads + kThreads - 1) / kThreads;          // <= 2^23 per level
  }
  msk_launch_scope ls(ctx, "label_pyramid");
  hipLaunchKernelGGL(label_pyramid_k, dim3(blocks), dim3(kThreads), 0, ctx->stream, label, t);
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
