/* The three region-based training entry points (medicalseg_amd/csrc/msk_loss_mlabel.hip) for the host-only STAND-IN library:
 * tests/test_mlabel_stack_host.py compiles this file together with tests/fake_msegk.c, tests/fake_msegk_region.c and
 * tests/fake_msegk_pyramid.c into one shared object.  Like those it computes NOTHING (the records stay as allocated: zeros);
 * the calls are counted and the last call's arguments are kept so that the test can see what the loss objects asked for. */
#include <stdint.h>

typedef struct { void* p; int32_t n, d, h, w, c, ld; } fake_tensor;

static long g_fwd = 0, g_bwd = 0, g_to_label = 0;
static int g_accumulate = -1, g_table_len = -1, g_squared = -1, g_batch_dice = -1, g_ignore = -1, g_regions = -1;
static float g_coef_bce = 0.f, g_coef_dice = 0.f, g_smooth = 0.f;
static uint32_t g_table[256];
static int32_t g_order[32];
static int g_label_shape[4];

long fake_mlabel_calls(int which) { return which == 0 ? g_fwd : which == 1 ? g_bwd : g_to_label; }
int fake_mlabel_last_int(int which) {
  return which == 0 ? g_accumulate : which == 1 ? g_table_len : which == 2 ? g_squared : which == 3 ? g_batch_dice : which == 4 ? g_ignore
                                                                                                                               : g_regions;
}
float fake_mlabel_last_float(int which) { return which == 0 ? g_coef_bce : which == 1 ? g_coef_dice : g_smooth; }
uint32_t fake_mlabel_table(int v) { return g_table[v]; }
int32_t fake_mlabel_order(int r) { return g_order[r]; }
int fake_mlabel_label_shape(int i) { return g_label_shape[i]; }

static void keep(fake_tensor logits, int ignore_index, const uint32_t* table, int table_len, int squared_pred, int batch_dice,
                 float smooth) {
  g_ignore = ignore_index;
  g_table_len = table_len;
  g_squared = squared_pred;
  g_batch_dice = batch_dice;
  g_smooth = smooth;
  g_regions = logits.c;
  for (int i = 0; i < 256; ++i) g_table[i] = (table && i < table_len) ? table[i] : 0u;   /* the stand-in's device memory is host memory */
}

int msk_mlabel_loss_fwd(void* ctx, fake_tensor logits, const int32_t* labels, int ignore_index, const uint32_t* table, int table_len,
                        int squared_pred, int batch_dice, float smooth, float* out, double* stats) {
  (void)ctx; (void)labels; (void)out; (void)stats;
  ++g_fwd;
  keep(logits, ignore_index, table, table_len, squared_pred, batch_dice, smooth);
  return 0;
}

int msk_mlabel_loss_bwd(void* ctx, fake_tensor logits, const int32_t* labels, int ignore_index, const uint32_t* table, int table_len,
                        int squared_pred, int batch_dice, float smooth, const double* stats, float coef_bce, float coef_dice,
                        int accumulate, fake_tensor dlogits) {
  (void)ctx; (void)labels; (void)stats; (void)dlogits;
  ++g_bwd;
  keep(logits, ignore_index, table, table_len, squared_pred, batch_dice, smooth);
  g_accumulate = accumulate;
  g_coef_bce = coef_bce;
  g_coef_dice = coef_dice;
  return 0;
}

int msk_regions_to_label(void* ctx, fake_tensor logits, const int32_t* class_order, int32_t* out) {
  (void)ctx; (void)out;
  ++g_to_label;
  g_regions = logits.c;
  g_label_shape[0] = logits.n; g_label_shape[1] = logits.d; g_label_shape[2] = logits.h; g_label_shape[3] = logits.w;
  for (int r = 0; r < 32; ++r) g_order[r] = r < logits.c ? class_order[r] : -1;
  return 0;
}

/* evaluate(hard_metrics=True) over the stand-in: the counts stay zero */
int msk_confusion3d() { return 0; }
