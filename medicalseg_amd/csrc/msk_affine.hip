// Rotated and scaled patch cropping (transforms.RandomAffinePatchCrop3D, tests/affine_reference.py): the sampling grid of a
// patch is built around the patch centre, turned and scaled by a 3x3 matrix, and the volume is read ONCE -- trilinear for the
// image, nearest neighbour for the label, both from the same coordinates.  The patch origin is the first three words of a
// msk_patch_select record and is read on the device, so nothing synchronises and nothing is downloaded.  The cost follows the
// patch, not the volume.
//
// Per output voxel (z, y, x), o = (z - rd/2, y - rh/2, x - rw/2), per source axis a:
//     p_a = ((M[a][0]*o_z + M[a][1]*o_y) + M[a][2]*o_x) + (float)(origin_a + roi_a/2)
// image: f = floor(p), t = p - f, the eight corners f + {0,1}^3 (pad outside the volume), lerp(a, b, t) = a + t*(b - a) along
// W, then H, then D; label: the voxel at floor(p + 0.5f), label_pad outside.  Every multiply and add is rounded on its own:
// the file is compiled under `#pragma clang fp contract(off)` (msk_sliding.hip's header has the evidence that __fmul_rn /
// __fadd_rn do not prevent fusion in this toolchain).  ISA of all four instantiations read after building for gfx950: the
// coordinate chain is v_mul_f32 / v_add_f32 and the seven lerps are v_sub_f32 / v_mul_f32 / v_add_f32; the kernels hold no
// v_fma_f32, v_fmac_f32 or v_mad_f32 at all.
//
// msk_affine_patch_elastic is the same voxel routine with one more template parameter: the three offsets are displaced by the
// field of msk_elastic_field (msk_elastic.hip) before the matrix, e_a = o_a + F_a, one add per axis (tests/elastic_reference.py).
// The instantiations without it are the code they were.
//
// One launch, one thread per output voxel, no atomics, no LDS.  A corner outside the volume is never loaded from there: its
// index is clamped into the volume (so all eight loads are unconditional and in flight together) and the value is replaced by
// the pad with a select.  Two thread -> voxel maps (context option "affine_map", A/B; DESIGN.md section 7 has both times):
//   1 (default)  a workgroup of 256 threads covers a 4 x 4 x 16 box of the patch, a wavefront 2 x 2 x 16 of it: four 64-byte
//                store segments per wavefront, and the source footprint of a wavefront is a compact box whatever the rotation
//   0            row-linear: consecutive threads on consecutive x of the flattened patch (256-byte store segments; a wavefront
//                reads along one oblique line of the volume)
#include "msk_common.h"

#pragma clang fp contract(off)   // for the whole file: no multiply below may be fused with an add

namespace {

constexpr int kThreads = 256;
constexpr int kMaxExtent = 8192;
constexpr float kMaxEntry = 4.0f;
constexpr int kTileZ = 4, kTileY = 4, kTileX = 16;   // patch box of one workgroup (tile map)
static_assert(kTileZ * kTileY * kTileX == kThreads, "one thread per voxel of the box");

struct AffineArgs {
  int D, H, W;      // source extent
  int rd, rh, rw;   // patch extent
  float m[9];       // row-major: source axis x patch axis
  float pad;
  int32_t label_pad;
};

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// kElastic: the offset is displaced by the field [3][rd][rh][rw] of msk_elastic_field before the matrix (batchgenerators'
// order: deform the zero-centred mesh, then rotate and scale it, then move it to the centre)
template <bool kLabel, bool kElastic>
__device__ __forceinline__ void affine_voxel(const float* __restrict__ img, const int32_t* __restrict__ label,
                                             const int32_t* __restrict__ sel, const float* __restrict__ field,
                                             float* __restrict__ out_img, int32_t* __restrict__ out_label, const AffineArgs& g,
                                             int z, int y, int x) {
  const float cd = (float)(sel[0] + g.rd / 2), ch = (float)(sel[1] + g.rh / 2), cw = (float)(sel[2] + g.rw / 2);
  float oz = (float)(z - g.rd / 2), oy = (float)(y - g.rh / 2), ox = (float)(x - g.rw / 2);
  const long o = ((long)z * g.rh + y) * g.rw + x;
  if (kElastic) {
    const long n = (long)g.rd * g.rh * g.rw;
    oz = oz + field[o];
    oy = oy + field[n + o];
    ox = ox + field[2 * n + o];
  }
  // without a field |o| <= 8192 and |p| <= 3 * 4 * 8192 + 2 * 8192 < 2^17; with msk_elastic_field's |F| <= 4096 (alpha <= 4096,
  // |smoothed u| <= 1 up to rounding) |e| <= 8192 + 4096 and |p| <= 3 * 4 * 12288 + 2 * 8192 < 2^18: the conversions below are
  // defined.  For any other field content (NaN and infinities included) v_cvt_i32_f32 saturates and every index is clamped
  // into the volume before it is used, so no address leaves the volume.
  const float pd = ((g.m[0] * oz + g.m[1] * oy) + g.m[2] * ox) + cd;
  const float ph = ((g.m[3] * oz + g.m[4] * oy) + g.m[5] * ox) + ch;
  const float pw = ((g.m[6] * oz + g.m[7] * oy) + g.m[8] * ox) + cw;
  const float fd = floorf(pd), fh = floorf(ph), fw = floorf(pw);
  const float td = pd - fd, th = ph - fh, tw = pw - fw;
  const int d0 = (int)fd, h0 = (int)fh, w0 = (int)fw;
  const int D1 = g.D - 1, H1 = g.H - 1, W1 = g.W - 1;
  const bool vd0 = (unsigned)d0 < (unsigned)g.D, vd1 = (unsigned)(d0 + 1) < (unsigned)g.D;
  const bool vh0 = (unsigned)h0 < (unsigned)g.H, vh1 = (unsigned)(h0 + 1) < (unsigned)g.H;
  const bool vw0 = (unsigned)w0 < (unsigned)g.W, vw1 = (unsigned)(w0 + 1) < (unsigned)g.W;
  // clamped: every address is inside the volume, whether the corner is or not
  const long rd0 = (long)clampi(d0, D1) * g.H, rd1 = (long)clampi(d0 + 1, D1) * g.H;
  const int hc0 = clampi(h0, H1), hc1 = clampi(h0 + 1, H1);
  const int wc0 = clampi(w0, W1), wc1 = clampi(w0 + 1, W1);
  const float* r00 = img + (rd0 + hc0) * g.W;
  const float* r01 = img + (rd0 + hc1) * g.W;
  const float* r10 = img + (rd1 + hc0) * g.W;
  const float* r11 = img + (rd1 + hc1) * g.W;
  const float l000 = r00[wc0], l001 = r00[wc1], l010 = r01[wc0], l011 = r01[wc1];
  const float l100 = r10[wc0], l101 = r10[wc1], l110 = r11[wc0], l111 = r11[wc1];
  int32_t lab = 0;
  bool lab_in = false;
  if (kLabel) {
    const int ld = (int)floorf(pd + 0.5f), lh = (int)floorf(ph + 0.5f), lw = (int)floorf(pw + 0.5f);
    lab_in = (unsigned)ld < (unsigned)g.D && (unsigned)lh < (unsigned)g.H && (unsigned)lw < (unsigned)g.W;
    lab = label[((long)clampi(ld, D1) * g.H + clampi(lh, H1)) * g.W + clampi(lw, W1)];
  }
  const float pad = g.pad;
  const float v000 = vd0 && vh0 && vw0 ? l000 : pad, v001 = vd0 && vh0 && vw1 ? l001 : pad;
  const float v010 = vd0 && vh1 && vw0 ? l010 : pad, v011 = vd0 && vh1 && vw1 ? l011 : pad;
  const float v100 = vd1 && vh0 && vw0 ? l100 : pad, v101 = vd1 && vh0 && vw1 ? l101 : pad;
  const float v110 = vd1 && vh1 && vw0 ? l110 : pad, v111 = vd1 && vh1 && vw1 ? l111 : pad;
  const float c00 = lerp(v000, v001, tw), c01 = lerp(v010, v011, tw);
  const float c10 = lerp(v100, v101, tw), c11 = lerp(v110, v111, tw);
  out_img[o] = lerp(lerp(c00, c01, th), lerp(c10, c11, th), td);
  if (kLabel) out_label[o] = lab_in ? lab : g.label_pad;
}

// row-linear: threads cover the flattened patch
template <bool kLabel, bool kElastic>
__global__ void __launch_bounds__(kThreads)
affine_rows_k(const float* __restrict__ img, const int32_t* __restrict__ label, const int32_t* __restrict__ sel,
              const float* __restrict__ field, float* __restrict__ out_img, int32_t* __restrict__ out_label, AffineArgs g) {
  const unsigned total = (unsigned)g.rd * (unsigned)g.rh * (unsigned)g.rw;
  const unsigned i = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  if (i >= total) return;
  const unsigned r = i / (unsigned)g.rw, x = i - r * (unsigned)g.rw;
  const unsigned z = r / (unsigned)g.rh, y = r - z * (unsigned)g.rh;
  affine_voxel<kLabel, kElastic>(img, label, sel, field, out_img, out_label, g, (int)z, (int)y, (int)x);
}

// tile: blockIdx.x = x box, blockIdx.y = y box, blockIdx.z = z box; lane bits 0-3 x, 4 y, 5 z, wavefront bits y, z
template <bool kLabel, bool kElastic>
__global__ void __launch_bounds__(kThreads)
affine_tile_k(const float* __restrict__ img, const int32_t* __restrict__ label, const int32_t* __restrict__ sel,
              const float* __restrict__ field, float* __restrict__ out_img, int32_t* __restrict__ out_label, AffineArgs g) {
  const int t = threadIdx.x;
  const int x = (int)blockIdx.x * kTileX + (t & 15);
  const int y = (int)blockIdx.y * kTileY + ((t >> 4) & 1) + ((t >> 6) & 1) * 2;
  const int z = (int)blockIdx.z * kTileZ + ((t >> 5) & 1) + ((t >> 7) & 1) * 2;
  if (x >= g.rw || y >= g.rh || z >= g.rd) return;
  affine_voxel<kLabel, kElastic>(img, label, sel, field, out_img, out_label, g, z, y, x);
}

inline bool extents_ok(int d, int h, int w) {
  return d >= 1 && h >= 1 && w >= 1 && d <= kMaxExtent && h <= kMaxExtent && w <= kMaxExtent;
}
template <bool kLabel, bool kElastic>
void launch_affine(msk_ctx* ctx, const float* img, const int32_t* label, const int32_t* sel, const float* field, float* out_img,
                   int32_t* out_label, const AffineArgs& g) {
  // grid.y and grid.z hold at most 8192 / 4 boxes
  const dim3 boxes((unsigned)msk_cdiv(g.rw, kTileX), (unsigned)msk_cdiv(g.rh, kTileY), (unsigned)msk_cdiv(g.rd, kTileZ));
  const dim3 rows((unsigned)msk_cdiv((long)g.rd * g.rh * g.rw, kThreads));
  if (ctx->affine_map != 0)
    hipLaunchKernelGGL((affine_tile_k<kLabel, kElastic>), boxes, dim3(kThreads), 0, ctx->stream, img, label, sel, field, out_img, out_label, g);
  else
    hipLaunchKernelGGL((affine_rows_k<kLabel, kElastic>), rows, dim3(kThreads), 0, ctx->stream, img, label, sel, field, out_img, out_label, g);
}

// msk_affine_patch (field == nullptr, elastic false) and msk_affine_patch_elastic: one set of checks, one voxel routine
int affine_patch(msk_ctx* ctx, const char* tag, bool elastic, const float* img, const int32_t* label, int d, int h, int w,
                 const int32_t* sel, const float* matrix, const float* field, float* out_img, int32_t* out_label, int rd, int rh,
                 int rw, float pad, int32_t label_pad) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, img != nullptr && sel != nullptr && matrix != nullptr && out_img != nullptr, "null img / sel / matrix / out_img");
  MSK_REQUIRE(ctx, (label != nullptr) == (out_label != nullptr), "label and out_label must both be set or both be null");
  MSK_REQUIRE(ctx, ((((uintptr_t)img) | ((uintptr_t)label) | ((uintptr_t)sel) | ((uintptr_t)out_img) | ((uintptr_t)out_label)) & 3) == 0,
              "img / label / sel / out_img / out_label must be 4-byte aligned");
  MSK_REQUIRE(ctx, extents_ok(d, h, w) && extents_ok(rd, rh, rw), "volume and patch extents must be in [1, 8192]");
  MSK_REQUIRE(ctx, msk_below_2_31(d, h, w) && msk_below_2_31(rd, rh, rw), "volume and patch must have fewer than 2^31 voxels each");
  AffineArgs g;
  for (int i = 0; i < 9; ++i) {
    // written so that a NaN fails: |m| <= 4 is false for it
    MSK_REQUIRE(ctx, matrix[i] >= -kMaxEntry && matrix[i] <= kMaxEntry, "matrix entries must be finite and inside [-4, 4]");
    g.m[i] = matrix[i];
  }
  const size_t vbytes = (size_t)d * h * w * 4, pbytes = (size_t)rd * rh * rw * 4;
  MSK_REQUIRE(ctx, msk_bytes_disjoint(out_img, pbytes, img, vbytes) && msk_bytes_disjoint(out_img, pbytes, sel, 12), "out_img must not overlap img or sel");
  if (label != nullptr) {
    MSK_REQUIRE(ctx, msk_bytes_disjoint(out_img, pbytes, label, vbytes), "out_img must not overlap label");
    MSK_REQUIRE(ctx, msk_bytes_disjoint(out_label, pbytes, img, vbytes) && msk_bytes_disjoint(out_label, pbytes, label, vbytes) &&
                         msk_bytes_disjoint(out_label, pbytes, sel, 12), "out_label must not overlap img, label or sel");
    MSK_REQUIRE(ctx, msk_bytes_disjoint(out_label, pbytes, out_img, pbytes), "out_label must not overlap out_img");
  }
  if (elastic) {
    MSK_REQUIRE(ctx, field != nullptr && (((uintptr_t)field) & 3) == 0, "field must be set and 4-byte aligned");
    MSK_REQUIRE(ctx, 3 * ((long)rd * rh * rw) <= 0x7fffffffL, "the field must have fewer than 2^31 elements");
    MSK_REQUIRE(ctx, msk_bytes_disjoint(out_img, pbytes, field, 3 * pbytes), "out_img must not overlap field");
    if (label != nullptr) MSK_REQUIRE(ctx, msk_bytes_disjoint(out_label, pbytes, field, 3 * pbytes), "out_label must not overlap field");
  }
  g.D = d; g.H = h; g.W = w;
  g.rd = rd; g.rh = rh; g.rw = rw;
  g.pad = pad;
  g.label_pad = label_pad;
  msk_launch_scope ls(ctx, tag);
  if (elastic) {
    if (label != nullptr) launch_affine<true, true>(ctx, img, label, sel, field, out_img, out_label, g);
    else launch_affine<false, true>(ctx, img, label, sel, field, out_img, out_label, g);
  } else {
    if (label != nullptr) launch_affine<true, false>(ctx, img, label, sel, field, out_img, out_label, g);
    else launch_affine<false, false>(ctx, img, label, sel, field, out_img, out_label, g);
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}
}  // namespace

extern "C" {

int msk_affine_patch(msk_ctx* ctx, const float* img, const int32_t* label, int d, int h, int w, const int32_t* sel,
                     const float* matrix, float* out_img, int32_t* out_label, int rd, int rh, int rw, float pad, int32_t label_pad) {
  return affine_patch(ctx, "affine_patch", false, img, label, d, h, w, sel, matrix, nullptr, out_img, out_label, rd, rh, rw, pad, label_pad);
}

int msk_affine_patch_elastic(msk_ctx* ctx, const float* img, const int32_t* label, int d, int h, int w, const int32_t* sel,
                             const float* matrix, const float* field, float* out_img, int32_t* out_label, int rd, int rh, int rw,
                             float pad, int32_t label_pad) {
  return affine_patch(ctx, "affine_patch_elastic", true, img, label, d, h, w, sel, matrix, field, out_img, out_label, rd, rh, rw, pad,
                      label_pad);
}

}  // extern "C"
