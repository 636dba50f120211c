// Foreground-oversampled random patch cropping (transforms.RandomPatchCrop3D, tests/patch_reference.py): choose "the r-th voxel
// of class c in raster order" of a label volume that lives on the device, turn it into a patch origin, and cut the patch out
// of image and label with implicit padding -- without a host synchronisation, a download or anything data-dependent on the
// host.  Integer arithmetic only; the only atomics are integer adds, so the result does not depend on scheduling.
//
// Three passes, all on the context stream:
//   histogram  one workgroup per CHUNK of kChunk = 4096 consecutive voxels (256 lanes x four 16-byte loads, issued together; a
//              scalar tail, and the scalar form for a label that is not 16-byte aligned).  Counts go into a 256-word LDS
//              histogram.  A label volume is mostly one class, so a wavefront first asks whether its 256 voxels of one load
//              hold ONE value and then adds 256 with a single LDS atomic; otherwise the four slots take the run-peeling of
//              msk_count_slot (msk_device.h, shared with msk_metrics.hip).  The workgroup writes its row of C
//              counters to the chunk table and adds its non-zero counters to the totals, one global atomic each.  The label
//              is read once; the table is C / 4096 of its size.
//   select     one workgroup per patch.  Class and rank follow from the totals and the patch's random words.  The class's
//              column of the chunk table is reduced to sums per SEGMENT of 64 chunks (one coalesced load and one wavefront
//              reduction each, four segments per wavefront in flight, no barrier in the loop), the segment is found with a
//              workgroup prefix sum over contiguous groups of segment sums, the chunk with a wavefront prefix sum over the
//              segment's 64 counters, and the voxel by re-reading that one chunk, 16 consecutive voxels per lane, with a
//              workgroup prefix sum over the per-lane match counts.  The 8-word record goes to sel.
//   crop       a thread per 16-byte quad of the patch (rw % 4 == 0) or per element; the origin is READ FROM sel on the
//              device, so whether a row start is a whole quad of the source (w0 % 4 == 0) is known only there: a branch
//              that is uniform over the launch picks 16-byte or 4-byte loads.  Elements are copied as 32-bit patterns.
// Every search is written so that an inconsistent table could only give another in-range voxel, never an out-of-range access.
#include "msk_common.h"

#include <climits>

namespace {

constexpr int kThreads = 256;
constexpr int kLaneVoxels = 16;
constexpr int kChunk = kThreads * kLaneVoxels;   // voxels per workgroup of the histogram pass = per row of the chunk table
constexpr int kSeg = 64;                          // chunks per segment: one per lane
constexpr int kMaxSeg = 8192;                     // 2^31 voxels / kChunk / kSeg
constexpr int kMaxClasses = 32;                   // candidate classes
constexpr int kMaxPatches = 16;
constexpr int kMaxNumClasses = 256;               // words of the LDS histogram == kThreads

static_assert(kMaxNumClasses == kThreads, "one lane per histogram word");
static_assert((long)kMaxSeg * kSeg * kChunk >= (1L << 31), "segment sums for every volume below 2^31 voxels");

__device__ __forceinline__ int class_key(int v, int C) { return (unsigned)v < (unsigned)C ? v : -1; }

// grid: one workgroup per chunk.  table: [chunks][C], totals: [C] (zeroed before the launch)
__global__ void __launch_bounds__(kThreads)
patch_hist_k(const int32_t* __restrict__ label, long V, int C, int vec, uint32_t* __restrict__ table, uint32_t* __restrict__ totals) {
  __shared__ uint32_t hist[kMaxNumClasses];
  const int t = threadIdx.x, lane = t & 63;
  hist[t] = 0;
  __syncthreads();
  const long base = (long)blockIdx.x * kChunk;
  const int n = (int)(V - base < (long)kChunk ? V - base : (long)kChunk);
  const int32_t* lab = label + base;
  const int nvec = vec ? n >> 2 : 0;
  if (nvec > 0) {
    const int4* l4 = reinterpret_cast<const int4*>(lab);
    int4 v[kLaneVoxels / 4];
    // a lane without a vector re-reads vector 0 (in range) and drops it: four unconditional loads, issued together
#pragma unroll
    for (int j = 0; j < kLaneVoxels / 4; ++j) {
      const int q = j * kThreads + t;
      v[j] = l4[q < nvec ? q : 0];
    }
#pragma unroll
    for (int j = 0; j < kLaneVoxels / 4; ++j) {
      if (j * kThreads + (t & ~63) >= nvec) continue;   // the same in every lane
      const int m = j * kThreads + t < nvec ? 0 : -1;   // or-ed into the keys: -1 = no voxel
      const int kx = class_key(v[j].x, C) | m, ky = class_key(v[j].y, C) | m, kz = class_key(v[j].z, C) | m,
                kw = class_key(v[j].w, C) | m;
      const int k0 = __builtin_amdgcn_readfirstlane(kx);
      if (__all(kx == k0 && ky == k0 && kz == k0 && kw == k0)) {   // 256 voxels of one value: one atomic, or none
        if (k0 >= 0 && lane == 0) atomicAdd(&hist[k0], 256u);
      } else {
        msk_count_slot(kx, hist, lane);
        msk_count_slot(ky, hist, lane);
        msk_count_slot(kz, hist, lane);
        msk_count_slot(kw, hist, lane);
      }
    }
  }
  for (int i0 = 4 * nvec + (t & ~63); i0 < n; i0 += kThreads) {   // i0: the same in every lane
    const int i = i0 + lane;
    msk_count_slot(i < n ? class_key(lab[i], C) : -1, hist, lane);
  }
  __syncthreads();
  if (t < C) {
    const uint32_t c = hist[t];
    table[(long)blockIdx.x * C + t] = c;
    if (c) atomicAdd(&totals[t], c);
  }
}

struct PatchSelArgs {
  int D, H, W, C;
  int rd, rh, rw;
  int n_classes;
  int nchunks, vec;
  long V;
  int classes[kMaxClasses];
  uint32_t words[kMaxPatches * 6];
};

__device__ __forceinline__ int pad_origin(int roi, int dim) { return -((roi - dim) / 2); }   // dim <= roi
__device__ __forceinline__ int centred_origin(int c, int roi, int dim) {
  if (dim <= roi) return pad_origin(roi, dim);
  int o = c - roi / 2;
  o = o < 0 ? 0 : o;
  return o > dim - roi ? dim - roi : o;
}
__device__ __forceinline__ int uniform_origin(uint32_t w, int roi, int dim) {
  if (dim <= roi) return pad_origin(roi, dim);
  return (int)(((unsigned long long)w * (unsigned long long)(dim - roi + 1)) >> 32);
}

// grid: one workgroup per patch
__global__ void __launch_bounds__(kThreads)
patch_select_k(const int32_t* __restrict__ label, const PatchSelArgs a, const uint32_t* __restrict__ table,
               const uint32_t* __restrict__ totals, int32_t* __restrict__ sel, int32_t* __restrict__ counts) {
  __shared__ uint32_t segsum[kMaxSeg];
  __shared__ uint32_t wsum[kThreads / 64];
  __shared__ uint32_t found[3];   // segment and rank inside it; voxel
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p = blockIdx.x, C = a.C;
  const uint32_t force = a.words[6 * p], w_cls = a.words[6 * p + 1], w_rank = a.words[6 * p + 2];
  if (counts != nullptr && p == 0 && t < C) counts[t] = (int32_t)totals[t];
  if (t < 3) found[t] = 0;
  int cls = -1;
  uint32_t cnt = 0;
  if (force != 0 && a.n_classes > 0) {   // the same in every thread, like everything that follows from it
    int m = 0;
    for (int i = 0; i < a.n_classes; ++i) m += totals[a.classes[i]] != 0;
    if (m > 0) {
      int k = (int)(((unsigned long long)w_cls * (unsigned long long)m) >> 32);
      for (int i = 0; i < a.n_classes; ++i) {
        const uint32_t tc = totals[a.classes[i]];
        if (tc == 0) continue;
        if (k == 0) { cls = a.classes[i]; cnt = tc; break; }
        --k;
      }
    }
  }
  int o0, o1, o2, cz = -1, cy = -1, cx = -1;
  if (cls < 0) {
    o0 = uniform_origin(a.words[6 * p + 3], a.rd, a.D);
    o1 = uniform_origin(a.words[6 * p + 4], a.rh, a.H);
    o2 = uniform_origin(a.words[6 * p + 5], a.rw, a.W);
  } else {
    const uint32_t r = (uint32_t)(((unsigned long long)w_rank * (unsigned long long)cnt) >> 32);   // < cnt
    const int nseg = (a.nchunks + kSeg - 1) / kSeg;
    // segment sums of the class's column: four segments per wavefront in flight
    for (int s0 = wave * 4; s0 < nseg; s0 += 4 * (kThreads / 64)) {
      uint32_t v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long ch = (long)(s0 + u) * kSeg + lane;
        v[u] = ch < a.nchunks ? table[ch * C + cls] : 0u;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t s = msk_wave_sum_u32(v[u]);
        if (lane == 0 && s0 + u < nseg) segsum[s0 + u] = s;
      }
    }
    __syncthreads();
    // the segment: thread t owns the segments [lo, hi)
    const int G = (nseg + kThreads - 1) / kThreads;
    const int lo = t * G < nseg ? t * G : nseg, hi = lo + G < nseg ? lo + G : nseg;
    uint32_t mine = 0;
    for (int s = lo; s < hi; ++s) mine += segsum[s];
    uint32_t excl = msk_block_excl_scan<false>(mine, 0u, msk_op_add(), wsum);
    if (r >= excl && r - excl < mine) {
      uint32_t rr = r - excl;
      int s = lo;
      while (s < hi - 1 && rr >= segsum[s]) rr -= segsum[s++];
      found[0] = (uint32_t)s;
      found[1] = rr;
    }
    __syncthreads();
    const int seg = (int)found[0];
    const uint32_t rr = found[1];
    // the chunk: every wavefront scans the segment's counters (the same result in each)
    const long ch = (long)seg * kSeg + lane;
    const uint32_t cv = ch < a.nchunks ? table[ch * C + cls] : 0u;
    const uint32_t cincl = msk_wave_incl_scan<false>(cv, msk_op_add());
    const unsigned long long hit = __ballot(rr >= cincl - cv && rr < cincl);
    const int hl = hit ? __ffsll((long long)hit) - 1 : 0;
    long chunk = (long)seg * kSeg + hl;
    if (chunk > a.nchunks - 1) chunk = a.nchunks - 1;
    const uint32_t r2 = rr - __shfl(cincl - cv, hl, 64);
    // the voxel: 16 consecutive voxels per thread, so thread order is raster order
    const long base = chunk * kChunk;
    const int n = (int)(a.V - base < (long)kChunk ? a.V - base : (long)kChunk);
    const int e0 = t * kLaneVoxels;
    int vals[kLaneVoxels];
    if (a.vec && e0 + kLaneVoxels <= n) {
      const int4* l4 = reinterpret_cast<const int4*>(label + base + e0);
#pragma unroll
      for (int j = 0; j < kLaneVoxels / 4; ++j) {
        const int4 q = l4[j];
        vals[4 * j] = q.x; vals[4 * j + 1] = q.y; vals[4 * j + 2] = q.z; vals[4 * j + 3] = q.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kLaneVoxels; ++k) vals[k] = e0 + k < n ? label[base + e0 + k] : -1;   // cls >= 0: -1 never matches
    }
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < kLaneVoxels; ++k) c += vals[k] == cls;
    excl = msk_block_excl_scan<false>(c, 0u, msk_op_add(), wsum);
    if (r2 >= excl && r2 - excl < c) {
      const uint32_t want = r2 - excl;
      uint32_t seen = 0;
      int kh = 0;
#pragma unroll
      for (int k = 0; k < kLaneVoxels; ++k) {
        if (vals[k] == cls) {
          if (seen == want) kh = k;
          ++seen;
        }
      }
      found[2] = (uint32_t)(base + e0 + kh);
    }
    __syncthreads();
    const uint32_t vox = found[2];
    const uint32_t hw = (uint32_t)a.H * (uint32_t)a.W;
    cz = (int)(vox / hw);
    const uint32_t rem = vox - (uint32_t)cz * hw;
    cy = (int)(rem / (uint32_t)a.W);
    cx = (int)(rem - (uint32_t)cy * (uint32_t)a.W);
    o0 = centred_origin(cz, a.rd, a.D);
    o1 = centred_origin(cy, a.rh, a.H);
    o2 = centred_origin(cx, a.rw, a.W);
  }
  if (t < 8) {
    const int rec = t == 0 ? o0 : t == 1 ? o1 : t == 2 ? o2 : t == 3 ? cls : t == 4 ? cz : t == 5 ? cy : t == 6 ? cx : 0;
    sel[8 * p + t] = rec;
  }
}

struct CropDims {
  int D, H, W;      // source extent
  int rd, rh, rw;   // patch extent
};

// patch quad <- source quad or padding; threads cover the whole patch
__global__ void __launch_bounds__(kThreads)
patch_crop_quad_k(const uint32_t* __restrict__ src, const int32_t* __restrict__ sel, uint32_t* __restrict__ dst, CropDims g,
                  uint32_t pad, int src_vec) {
  const unsigned rq = (unsigned)g.rw >> 2;
  const unsigned total = (unsigned)g.rd * (unsigned)g.rh * rq;
  const unsigned i = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  if (i >= total) return;
  const int d0 = sel[0], h0 = sel[1], w0 = sel[2];
  const bool quads = src_vec && (w0 & 3) == 0;   // the same in every thread of the launch
  const unsigned r = i / rq, q = i - r * rq;
  const unsigned z = r / (unsigned)g.rh, y = r - z * (unsigned)g.rh;
  const long d = (long)d0 + z, h = (long)h0 + y;
  const long s = (long)w0 + 4L * q;              // first element of the quad inside the source row (may be < 0)
  uint4 v = make_uint4(pad, pad, pad, pad);
  if (d >= 0 && d < g.D && h >= 0 && h < g.H) {
    const uint32_t* row = src + (d * g.H + h) * g.W;
    if (quads && s >= 0 && s + 3 < g.W) {
      v = *reinterpret_cast<const uint4*>(row + s);
    } else {
      if (s >= 0 && s < g.W) v.x = row[s];
      if (s + 1 >= 0 && s + 1 < g.W) v.y = row[s + 1];
      if (s + 2 >= 0 && s + 2 < g.W) v.z = row[s + 2];
      if (s + 3 >= 0 && s + 3 < g.W) v.w = row[s + 3];
    }
  }
  reinterpret_cast<uint4*>(dst)[i] = v;
}

// any rw, any alignment: one thread per element
__global__ void __launch_bounds__(kThreads)
patch_crop_elem_k(const uint32_t* __restrict__ src, const int32_t* __restrict__ sel, uint32_t* __restrict__ dst, CropDims g,
                  uint32_t pad) {
  const unsigned total = (unsigned)g.rd * (unsigned)g.rh * (unsigned)g.rw;
  const unsigned i = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  if (i >= total) return;
  const int d0 = sel[0], h0 = sel[1], w0 = sel[2];
  const unsigned r = i / (unsigned)g.rw, x = i - r * (unsigned)g.rw;
  const unsigned z = r / (unsigned)g.rh, y = r - z * (unsigned)g.rh;
  const long d = (long)d0 + z, h = (long)h0 + y, w = (long)w0 + x;
  uint32_t v = pad;
  if (d >= 0 && d < g.D && h >= 0 && h < g.H && w >= 0 && w < g.W) v = src[(d * g.H + h) * g.W + w];
  dst[i] = v;
}

inline long chunks_of(long voxels) { return (voxels + kChunk - 1) / kChunk; }
inline bool extents_ok(int d, int h, int w) { return d >= 1 && h >= 1 && w >= 1; }

}  // namespace

extern "C" {

int msk_patch_workspace(long voxels, int num_classes, size_t* bytes) {
  MSK_REQUIRE(nullptr, bytes != nullptr, "bytes must not be null");
  MSK_REQUIRE(nullptr, voxels >= 1 && voxels <= 0x7fffffffL, "voxels must be in [1, 2^31)");
  MSK_REQUIRE(nullptr, num_classes >= 1 && num_classes <= kMaxNumClasses, "num_classes must be in [1, 256]");
  // the totals, then one row of num_classes counters per chunk
  const size_t words = (size_t)num_classes * (size_t)(chunks_of(voxels) + 1);
  *bytes = (words * sizeof(uint32_t) + 255) & ~(size_t)255;
  return 0;
}

int msk_patch_select(msk_ctx* ctx, const int32_t* label, int d, int h, int w, int num_classes, const int32_t* classes, int n_classes,
                     int rd, int rh, int rw, const uint32_t* words, int n_patches, void* workspace, int32_t* sel, int32_t* counts) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, label != nullptr && words != nullptr && workspace != nullptr && sel != nullptr, "null label / words / workspace / sel");
  MSK_REQUIRE(ctx, ((((uintptr_t)label) | ((uintptr_t)workspace) | ((uintptr_t)sel) | ((uintptr_t)counts)) & 3) == 0,
              "label / workspace / sel / counts must be 4-byte aligned");
  MSK_REQUIRE(ctx, extents_ok(d, h, w) && extents_ok(rd, rh, rw), "volume and patch extents must be >= 1");
  MSK_REQUIRE(ctx, msk_below_2_31(d, h, w), "the volume must have fewer than 2^31 voxels");
  MSK_REQUIRE(ctx, num_classes >= 1 && num_classes <= kMaxNumClasses, "num_classes must be in [1, 256]");
  MSK_REQUIRE(ctx, n_classes >= 0 && n_classes <= kMaxClasses, "n_classes must be in [0, 32]");
  MSK_REQUIRE(ctx, n_classes == 0 || classes != nullptr, "classes must be a host array of n_classes int32");
  MSK_REQUIRE(ctx, n_patches >= 1 && n_patches <= kMaxPatches, "n_patches must be in [1, 16]");
  PatchSelArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n_classes; ++i) {
    MSK_REQUIRE(ctx, classes[i] >= 0 && classes[i] < num_classes, "classes: a class outside [0, num_classes)");
    MSK_REQUIRE(ctx, i == 0 || classes[i] > classes[i - 1], "classes must be strictly ascending");
    a.classes[i] = classes[i];
  }
  bool forced = false;
  for (int i = 0; i < 6 * n_patches; ++i) a.words[i] = words[i];
  for (int p = 0; p < n_patches; ++p) forced = forced || words[6 * p] != 0;
  a.D = d; a.H = h; a.W = w; a.C = num_classes;
  a.rd = rd; a.rh = rh; a.rw = rw;
  a.n_classes = n_classes;
  a.V = (long)d * h * w;
  a.nchunks = (int)chunks_of(a.V);
  a.vec = (((uintptr_t)label) & 15) == 0;
  uint32_t* totals = (uint32_t*)workspace;
  uint32_t* table = totals + num_classes;
  // a call in which no patch can take the foreground branch and nobody asks for the counts needs no histogram
  if (counts != nullptr || (forced && n_classes > 0)) {
    MSK_CHECK_HIP(ctx, hipMemsetAsync(totals, 0, (size_t)num_classes * sizeof(uint32_t), ctx->stream));
    msk_launch_scope ls(ctx, "patch_hist");
    hipLaunchKernelGGL(patch_hist_k, dim3((unsigned)a.nchunks), dim3(kThreads), 0, ctx->stream, label, a.V, num_classes, a.vec, table,
                       totals);
  }
  {
    msk_launch_scope ls(ctx, "patch_select");
    hipLaunchKernelGGL(patch_select_k, dim3((unsigned)n_patches), dim3(kThreads), 0, ctx->stream, label, a, (const uint32_t*)table,
                       (const uint32_t*)totals, sel, counts);
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

int msk_patch_crop(msk_ctx* ctx, const void* src, int d, int h, int w, const int32_t* sel, void* dst, int rd, int rh, int rw,
                   uint32_t pad_bits) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, src != nullptr && sel != nullptr && dst != nullptr, "null src / sel / dst");
  MSK_REQUIRE(ctx, ((((uintptr_t)src) | ((uintptr_t)sel) | ((uintptr_t)dst)) & 3) == 0, "src / sel / dst must be 4-byte aligned");
  MSK_REQUIRE(ctx, extents_ok(d, h, w) && extents_ok(rd, rh, rw), "volume and patch extents must be >= 1");
  MSK_REQUIRE(ctx, msk_below_2_31(d, h, w) && msk_below_2_31(rd, rh, rw), "volume and patch must have fewer than 2^31 voxels each");
  const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)d * h * w * 4, d0 = (uintptr_t)dst, d1 = d0 + (size_t)rd * rh * rw * 4;
  MSK_REQUIRE(ctx, s1 <= d0 || d1 <= s0, "dst must not overlap src");
  CropDims g;
  g.D = d; g.H = h; g.W = w;
  g.rd = rd; g.rh = rh; g.rw = rw;
  msk_launch_scope ls(ctx, "patch_crop");
  if (rw % 4 == 0 && (d0 & 15) == 0) {
    const long total = (long)rd * rh * (rw / 4);
    const int src_vec = (s0 & 15) == 0 && w % 4 == 0;
    hipLaunchKernelGGL(patch_crop_quad_k, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream,
                       (const uint32_t*)src, sel, (uint32_t*)dst, g, pad_bits, src_vec);
  } else {
    const long total = (long)rd * rh * rw;
    hipLaunchKernelGGL(patch_crop_elem_k, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream,
                       (const uint32_t*)src, sel, (uint32_t*)dst, g, pad_bits);
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
