/* The Lovasz-Softmax entry points (medicalseg_amd/csrc/msk_loss_lovasz.hip) for the host-only STAND-IN library:
 * tests/test_lovasz_stack_host.py compiles this file together with tests/fake_msegk.c, tests/fake_msegk_region.c and
 * tests/fake_msegk_pyramid.c into one shared object.  Like those it computes NOTHING (the records stay as allocated: zeros); the
 * calls are counted and the last calls' arguments are kept so that the test can see what the loss objects asked for. */
#include <stddef.h>
#include <stdint.h>

typedef struct { void* p; int32_t n, d, h, w, c, ld; } fake_tensor;

static long g_ws = 0, g_fwd = 0, g_bwd = 0;
static long g_ws_voxels = 0;
static int g_ws_classes = -1, g_ws_groups = -1;
static int g_accumulate = -1, g_ignore = -1, g_mode = -1, g_per_image = -1, g_bwd_per_image = -1;
static unsigned long long g_mask = 0;
static size_t g_fwd_bytes = 0, g_bwd_bytes = 0;
static float g_coef = 0.f;
static const void *g_fwd_ws = 0, *g_bwd_ws = 0, *g_fwd_stats = 0, *g_bwd_stats = 0, *g_labels = 0, *g_out = 0;

/* 0: workspace queries, 1: forward calls, 2: backward calls */
long fake_lovasz_calls(int which) { return which == 0 ? g_ws : which == 1 ? g_fwd : g_bwd; }
/* the last workspace query: 0 voxels of a group, 1 classes, 2 groups */
long fake_lovasz_ws_arg(int which) { return which == 0 ? g_ws_voxels : which == 1 ? g_ws_classes : g_ws_groups; }
/* 0: the last backward's accumulate, 1: the last forward's ignore_index, 2: its class_mode, 3: its per_image, 4: the last
 * backward's per_image */
int fake_lovasz_last_int(int which) {
  return which == 0 ? g_accumulate : which == 1 ? g_ignore : which == 2 ? g_mode : which == 3 ? g_per_image : g_bwd_per_image;
}
unsigned long long fake_lovasz_last_mask(void) { return g_mask; }
float fake_lovasz_last_coef(void) { return g_coef; }
/* workspace_bytes of the last forward (0) / backward (1) */
size_t fake_lovasz_last_bytes(int which) { return which == 0 ? g_fwd_bytes : g_bwd_bytes; }
/* 0 / 1: workspace of the last forward / backward, 2 / 3: their records, 4: the last forward's labels, 5: its out */
const void* fake_lovasz_last_ptr(int which) {
  return which == 0 ? g_fwd_ws : which == 1 ? g_bwd_ws : which == 2 ? g_fwd_stats : which == 3 ? g_bwd_stats : which == 4 ? g_labels : g_out;
}

int msk_lovasz_workspace(long voxels, int classes, int groups, size_t* bytes) {
  if (!bytes || voxels < 1 || classes < 2 || groups < 1) return -1;
  ++g_ws;
  g_ws_voxels = voxels;
  g_ws_classes = classes;
  g_ws_groups = groups;
  *bytes = (size_t)voxels * classes * groups * 16 + 8192;
  return 0;
}

int msk_lovasz_fwd(void* ctx, fake_tensor logits, const int32_t* labels, int ignore_index, int class_mode,
                   unsigned long long class_mask, int per_image, void* workspace, size_t workspace_bytes, float* out, double* stats) {
  (void)ctx; (void)logits;
  ++g_fwd;
  g_labels = labels;
  g_ignore = ignore_index;
  g_mode = class_mode;
  g_mask = class_mask;
  g_per_image = per_image;
  g_fwd_ws = workspace;
  g_fwd_bytes = workspace_bytes;
  g_out = out;
  g_fwd_stats = stats;
  return 0;
}

int msk_lovasz_bwd(void* ctx, fake_tensor logits, const int32_t* labels, int ignore_index, int per_image, const void* workspace,
                   size_t workspace_bytes, const double* stats, float coef, int accumulate, fake_tensor dz) {
  (void)ctx; (void)logits; (void)labels; (void)ignore_index; (void)dz;
  ++g_bwd;
  g_bwd_per_image = per_image;
  g_bwd_ws = workspace;
  g_bwd_bytes = workspace_bytes;
  g_bwd_stats = stats;
  g_coef = coef;
  g_accumulate = accumulate;
  return 0;
}
