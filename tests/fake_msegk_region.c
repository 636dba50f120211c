/* The two region-loss entry points (medicalseg_amd/csrc/msk_loss_region.hip) for the host-only STAND-IN library:
 * tests/test_region_host.py compiles this file together with tests/fake_msegk.c into one shared object.  Like that file it
 * computes NOTHING (the records stay as allocated: zeros); the calls are counted and the last backward call's `accumulate`
 * and coefficients are kept so that the test can see what the loss objects asked for. */
#include <stdint.h>

typedef struct { void* p; int32_t n, d, h, w, c, ld; } fake_tensor;

static long g_fwd = 0, g_bwd = 0;
static int g_accumulate = -1, g_focal_on = -1, g_batch_dice = -1, g_mode = -1;
static float g_coef_f = 0.f, g_coef_r = 0.f;

long fake_region_calls(int which) { return which == 0 ? g_fwd : g_bwd; }
int fake_region_last_int(int which) { return which == 0 ? g_accumulate : which == 1 ? g_focal_on : which == 2 ? g_batch_dice : g_mode; }
float fake_region_last_coef(int which) { return which == 0 ? g_coef_f : g_coef_r; }

int msk_region_loss_fwd(void* ctx, fake_tensor logits, const int32_t* labels, int ignore_index, int activation, int squared_pred,
                        int batch_dice, int do_bg, int mode, float smooth, float alpha, float beta, int focal_on, float gamma,
                        const float* weight, float* out, double* stats) {
  (void)ctx; (void)logits; (void)labels; (void)ignore_index; (void)activation; (void)squared_pred; (void)do_bg; (void)smooth;
  (void)alpha; (void)beta; (void)gamma; (void)weight; (void)out; (void)stats;
  ++g_fwd;
  g_focal_on = focal_on;
  g_batch_dice = batch_dice;
  g_mode = mode;
  return 0;
}

int msk_region_loss_bwd(void* ctx, fake_tensor logits, const int32_t* labels, int ignore_index, int activation, int squared_pred,
                        int batch_dice, int do_bg, int mode, float smooth, float alpha, float beta, int focal_on, float gamma,
                        const float* weight, const double* stats, float coef_f, float coef_r, int accumulate, fake_tensor dlogits) {
  (void)ctx; (void)logits; (void)labels; (void)ignore_index; (void)activation; (void)squared_pred; (void)batch_dice; (void)do_bg;
  (void)mode; (void)smooth; (void)alpha; (void)beta; (void)focal_on; (void)gamma; (void)weight; (void)stats; (void)dlogits;
  ++g_bwd;
  g_accumulate = accumulate;
  g_coef_f = coef_f;
  g_coef_r = coef_r;
  return 0;
}
