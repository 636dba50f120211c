// Confusion counts of a hard-label prediction against its label: the integers every metric of the reference's
// utils/metric.py (calculate_area -> mean_iou / dice / accuracy / kappa) is a sum of.
//
// Per volume a histogram over B = K*K + 1 bins, K = num_classes + 1: bin r*K + c = label class r, predicted class c
// (class num_classes = "other": negative or >= num_classes), the last bin = label == ignore_index.  One pass over the
// two int32 streams; counts are integers, so the result is exact and does not depend on the order of the adds.
//
// Aggregation (three levels, integer atomics only):
//   wavefront: a slot is one voxel per lane, and msk_count_slot (msk_device.h) adds a slot to the LDS histogram with one
//     atomic per run of equal keys.  One bin: 1 round and no per-lane atomic; 5 % foreground blobs: 1-2 rounds; 441 uniformly
//     random bins: 2 short rounds + the per-lane adds.
//   workgroup: a 32-bit histogram in LDS (a workgroup sees far fewer than 2^32 voxels);
//   grid: one 64-bit global atomic per non-zero bin per workgroup.
//
// Loads are 16 bytes per lane where both pointers of a volume reach 16-byte alignment after the same number of
// elements (always, for the volumes of one tensor pair with equal offsets); the head before that point and the tail
// behind the last whole vector go one element per lane, as does a whole volume whose two pointers disagree.
#include "msk_common.h"

namespace {

constexpr int kThreads = 256;
constexpr long kBlockVoxels = 8192;   // least voxels per workgroup: bounds the global atomics (B per workgroup) of a small volume

__device__ __forceinline__ int conf_key(int lab, int prd, int C, int K, int ignore_index) {
  const int r = (unsigned)lab < (unsigned)C ? lab : C;
  const int c = (unsigned)prd < (unsigned)C ? prd : C;
  return lab == ignore_index ? K * K : r * K + c;
}

// elements [a, b) of one volume, one per lane, strided over the volume's workgroups
__device__ __forceinline__ void count_range(const int32_t* __restrict__ prd, const int32_t* __restrict__ lab, long a, long b,
                                            long stride, int C, int K, int ignore_index, uint32_t* __restrict__ hist,
                                            int lane) {
  for (long i0 = a + (long)blockIdx.x * kThreads + (threadIdx.x & ~63); i0 < b; i0 += stride) {   // i0: the same in every lane
    const long i = i0 + lane;
    const int key = i < b ? conf_key(lab[i], prd[i], C, K, ignore_index) : -1;
    msk_count_slot(key, hist, lane);
  }
}

// grid (workgroups per volume, n); dynamic LDS: B 32-bit words
__global__ void __launch_bounds__(kThreads)
confusion_k(const int32_t* __restrict__ pred, const int32_t* __restrict__ label, long V, int C, int ignore_index,
            unsigned long long* __restrict__ counts) {
  extern __shared__ uint32_t hist[];
  const int K = C + 1, B = K * K + 1;
  const int t = threadIdx.x, lane = t & 63;
  for (int b = t; b < B; b += kThreads) hist[b] = 0;
  __syncthreads();
  const int32_t* prd = pred + (long)blockIdx.y * V;
  const int32_t* lab = label + (long)blockIdx.y * V;
  const unsigned mp = (unsigned)(((uintptr_t)prd >> 2) & 3), ml = (unsigned)(((uintptr_t)lab >> 2) & 3);
  long head = mp == ml ? (long)((4 - mp) & 3) : V;   // elements in front of the first 16-byte boundary of both streams
  if (head > V) head = V;
  const long nvec = (V - head) >> 2;
  const long stride = (long)gridDim.x * kThreads;
  const int4* p4 = reinterpret_cast<const int4*>(prd + head);
  const int4* l4 = reinterpret_cast<const int4*>(lab + head);
  // two vectors of each stream per lane in flight
  for (long q0 = (long)blockIdx.x * kThreads + (t & ~63); q0 < nvec; q0 += 2 * stride) {
    const long qa = q0 + lane, qb = qa + stride;
    const bool va = qa < nvec, vb = qb < nvec;
    // a lane without a vector re-reads vector q0 (in range) and drops it: four unconditional loads, issued together
    const long ia = va ? qa : q0, ib = vb ? qb : q0;
    const int4 pa = p4[ia], la = l4[ia], pb = p4[ib], lb = l4[ib];
    const int ma = va ? 0 : -1, mb = vb ? 0 : -1;   // or-ed into the keys: -1 = no voxel
    msk_count_slot(conf_key(la.x, pa.x, C, K, ignore_index) | ma, hist, lane);
    msk_count_slot(conf_key(la.y, pa.y, C, K, ignore_index) | ma, hist, lane);
    msk_count_slot(conf_key(la.z, pa.z, C, K, ignore_index) | ma, hist, lane);
    msk_count_slot(conf_key(la.w, pa.w, C, K, ignore_index) | ma, hist, lane);
    if (q0 + stride < nvec) {   // the same in every lane
      msk_count_slot(conf_key(lb.x, pb.x, C, K, ignore_index) | mb, hist, lane);
      msk_count_slot(conf_key(lb.y, pb.y, C, K, ignore_index) | mb, hist, lane);
      msk_count_slot(conf_key(lb.z, pb.z, C, K, ignore_index) | mb, hist, lane);
      msk_count_slot(conf_key(lb.w, pb.w, C, K, ignore_index) | mb, hist, lane);
    }
  }
  count_range(prd, lab, 0, head, stride, C, K, ignore_index, hist, lane);
  count_range(prd, lab, head + 4 * nvec, V, stride, C, K, ignore_index, hist, lane);
  __syncthreads();
  unsigned long long* row = counts + (long)blockIdx.y * B;
  for (int b = t; b < B; b += kThreads) {
    const uint32_t c = hist[b];
    if (c) atomicAdd(&row[b], (unsigned long long)c);
  }
}

}  // namespace

extern "C" {

int msk_confusion3d(msk_ctx* ctx, const int32_t* pred, const int32_t* label, int n, long voxels_per_volume, int num_classes,
                    int ignore_index, unsigned long long* counts, int accumulate) {
  const int C = num_classes, K = C + 1, B = K * K + 1;
  const long V = voxels_per_volume;
  MSK_REQUIRE(ctx, C >= 1 && C <= 64, "num_classes must be in [1,64]");
  MSK_REQUIRE(ctx, n >= 1 && n <= 65535, "n must be in [1, 65535]");
  MSK_REQUIRE(ctx, V >= 1 && V <= 0x7fffffffL, "voxels_per_volume must be in [1, 2^31)");
  MSK_REQUIRE(ctx, pred != nullptr && label != nullptr && counts != nullptr, "null pred / label / counts");
  MSK_REQUIRE(ctx, ((((uintptr_t)pred) | ((uintptr_t)label)) & 3) == 0 && (((uintptr_t)counts) & 7) == 0,
              "pred / label must be 4-byte aligned, counts 8-byte aligned");
  if (!accumulate) MSK_CHECK_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)n * B * sizeof(unsigned long long), ctx->stream));
  // workgroups per volume: a fixed function of the shape and the device, about 8 per CU over all volumes
  long bx = (V + kBlockVoxels - 1) / kBlockVoxels;
  const long cap = 8L * ctx->num_cu / n > 1 ? 8L * ctx->num_cu / n : 1;
  if (bx > cap) bx = cap;
  msk_launch_scope ls(ctx, "confusion3d");
  hipLaunchKernelGGL(confusion_k, dim3((unsigned)bx, (unsigned)n), dim3(kThreads), (size_t)B * sizeof(uint32_t), ctx->stream,
                     pred, label, V, C, ignore_index, counts);
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
