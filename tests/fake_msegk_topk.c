/* The top-k entry points (medicalseg_amd/csrc/msk_loss_topk.hip) for the host-only STAND-IN library: tests/test_topk_host.py
 * compiles this file together with tests/fake_msegk.c and tests/fake_msegk_region.c into one shared object.  Like those it
 * computes NOTHING (the records stay as allocated: zeros); the calls are counted and the last calls' arguments are kept so that
 * the test can see what the loss objects asked for. */
#include <stddef.h>
#include <stdint.h>

typedef struct { void* p; int32_t n, d, h, w, c, ld; } fake_tensor;

static long g_ws = 0, g_select = 0, g_fwd = 0, g_bwd = 0;
static long g_ws_n = 0;
static int g_accumulate = -1, g_ignore = -1;
static float g_k = 0.f, g_coef = 0.f;
static const void *g_fwd_ws = 0, *g_bwd_ws = 0, *g_fwd_rec = 0, *g_bwd_rec = 0, *g_weights = 0, *g_labels = 0;

/* 0: workspace queries, 1: selects, 2: forward calls, 3: backward calls */
long fake_topk_calls(int which) { return which == 0 ? g_ws : which == 1 ? g_select : which == 2 ? g_fwd : g_bwd; }
long fake_topk_ws_n(void) { return g_ws_n; }
/* 0: the last backward's accumulate, 1: the last forward's ignore_index */
int fake_topk_last_int(int which) { return which == 0 ? g_accumulate : g_ignore; }
/* 0: the last forward's k_percent, 1: the last backward's coef */
float fake_topk_last_float(int which) { return which == 0 ? g_k : g_coef; }
/* 0 / 1: workspace of the last forward / backward, 2 / 3: their records, 4: the last forward's weights, 5: its labels */
const void* fake_topk_last_ptr(int which) {
  return which == 0 ? g_fwd_ws : which == 1 ? g_bwd_ws : which == 2 ? g_fwd_rec : which == 3 ? g_bwd_rec : which == 4 ? g_weights : g_labels;
}

int msk_topk_workspace(long n, size_t* bytes) {
  if (!bytes || n < 1) return -1;
  ++g_ws;
  g_ws_n = n;
  *bytes = (size_t)n * 4 + 8192;
  return 0;
}

int msk_topk_select(void* ctx, const float* x, long n, long k, void* workspace, double* record) {
  (void)ctx; (void)x; (void)n; (void)k; (void)workspace; (void)record;
  ++g_select;
  return 0;
}

int msk_topk_ce_fwd(void* ctx, fake_tensor logits, const int32_t* labels, int ignore_index, const float* weights, float k_percent,
                    void* workspace, float* out, double* record) {
  (void)ctx; (void)logits; (void)out;
  ++g_fwd;
  g_labels = labels;
  g_ignore = ignore_index;
  g_weights = weights;
  g_k = k_percent;
  g_fwd_ws = workspace;
  g_fwd_rec = record;
  return 0;
}

int msk_topk_ce_bwd(void* ctx, fake_tensor logits, const int32_t* labels, int ignore_index, const float* weights,
                    const void* workspace, const double* record, float coef, int accumulate, fake_tensor dz) {
  (void)ctx; (void)logits; (void)labels; (void)ignore_index; (void)weights; (void)dz;
  ++g_bwd;
  g_bwd_ws = workspace;
  g_bwd_rec = record;
  g_coef = coef;
  g_accumulate = accumulate;
  return 0;
}
