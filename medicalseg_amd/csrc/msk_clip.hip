// Gradient clipping for the optimizers (optimizer.Momentum / SGD / Adam with grad_clip=ClipGradByGlobalNorm / ClipGradByValue,
// Momentum with use_nesterov=True; tests/clip_reference.py is the statement).  All gradients live in one flat arena, so the
// global L2 norm is one streaming reduction over it whose result STAYS on the device: the update kernel reads the clip
// coefficient from a device record.  Nothing here synchronises, downloads or uses an atomic.
//
//   coef    the fixed-order float64 reduction of msk_device.h (msk_red_chunk / msk_red_finish, the one msk_intensity_stats uses),
//           sum of squares only: one wavefront per chunk of 4096 gradients, the chunk values go to the workspace (8 bytes per
//           16 KiB of gradient), and the finish pass -- one workgroup of 256 -- reduces them and one thread writes the record
//           {S, norm, coef, 0}: sqrt and the division are IEEE float64 operations.
//   update  msk_sgd_momentum_clip / msk_adam_clip (msk_loss_optim.hip, beside the plain entry points: one kernel each) read the
//           clip coefficient from that record.
#include <cmath>

#include "msk_common.h"

namespace {

// grid: one wavefront (64 threads) per chunk; g is 16-byte aligned.  At most four wavefronts per SIMD: the scheduler may then spend
// the registers that hold all 16 loads of a thread before the first add (aiming at seven, it starts to add behind the eighth)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 4)))
clip_chunk_k(const float* __restrict__ g, long n, double* __restrict__ psq) {
  const msk_red_vals r = msk_red_chunk<false>(g, n, true);
  if (threadIdx.x == 0) psq[blockIdx.x] = r.sumsq;
}

// one workgroup of 256; thread 0 writes the record
__global__ void __launch_bounds__(kMskRedLanes)
clip_finish_k(long nc, const double* __restrict__ psq, float grad_scale, float clip_norm, double* __restrict__ rec) {
  const msk_red_vals r = msk_red_finish<false>(nc, nullptr, psq, nullptr, nullptr);
  if (threadIdx.x == 0) {
    const double S = r.sumsq;
    const double cn = (double)clip_norm;
    const double norm = (double)grad_scale * sqrt(S);
    // cn / (norm > cn ? norm : cn) for a finite cn; an infinite cn measures only.  A NaN norm compares false: coef 1
    const float coef = norm > cn ? (float)(cn / norm) : 1.0f;
    rec[0] = S;
    rec[1] = norm;
    rec[2] = (double)coef;
    rec[3] = 0.0;
  }
}

}  // namespace

extern "C" {

int msk_grad_clip_workspace(size_t count, size_t* bytes) {
  MSK_REQUIRE(nullptr, bytes != nullptr, "bytes must not be null");
  MSK_REQUIRE(nullptr, count >= 1 && count <= (size_t)0x7fffffff, "count must be in [1, 2^31)");
  *bytes = (size_t)msk_chunks_of(count) * 8;
  return 0;
}

int msk_grad_clip_coef(msk_ctx* ctx, const float* grad, size_t count, float grad_scale, float clip_norm, void* workspace,
                       double* rec) {
  MSK_REQUIRE(ctx, ctx != nullptr, "null context");
  MSK_REQUIRE(ctx, grad != nullptr && workspace != nullptr && rec != nullptr, "null grad / workspace / rec");
  MSK_REQUIRE(ctx, count >= 1 && count <= (size_t)0x7fffffff, "count must be in [1, 2^31)");
  MSK_REQUIRE(ctx, clip_norm > 0.f, "clip_norm must be > 0 (+inf measures only)");   // a NaN compares false
  MSK_REQUIRE(ctx, (((uintptr_t)grad) & 15) == 0, "grad must be 16-byte aligned");
  MSK_REQUIRE(ctx, ((((uintptr_t)workspace) | ((uintptr_t)rec)) & 7) == 0, "workspace / rec must be 8-byte aligned");
  if (msk_join_side_impl(ctx) != 0) return -1;   // weight gradients (the late in_tr.conv1 one included) may still be running on the side stream
  const long nc = msk_chunks_of(count);
  double* psq = (double*)workspace;
  {
    msk_launch_scope ls(ctx, "grad_clip_chunks");
    hipLaunchKernelGGL(clip_chunk_k, dim3((unsigned)nc), dim3(64), 0, ctx->stream, grad, (long)count, psq);
  }
  {
    msk_launch_scope ls(ctx, "grad_clip_finish");
    hipLaunchKernelGGL(clip_finish_k, dim3(1), dim3(kMskRedLanes), 0, ctx->stream, nc, (const double*)psq, grad_scale, clip_norm, rec);
  }
  MSK_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
