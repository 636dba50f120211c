/* msk_label_pyramid (medicalseg_amd/csrc/msk_pyramid.hip) for the host-only STAND-IN library: tests/test_pyramid_host.py compiles
 * this file together with tests/fake_msegk.c and tests/fake_msegk_region.c into one shared object.  Like those it computes
 * NOTHING (the levels stay as allocated); the calls are counted and the last call's arguments are kept so that the test can
 * see what the loss objects asked for. */
#include <stdint.h>

static long g_calls = 0;
static int g_levels = 0;
static int g_shape[4];
static int g_extents[24];
static const void* g_label = 0;
static void* g_dst[8];

long fake_pyramid_calls(void) { return g_calls; }
int fake_pyramid_levels(void) { return g_levels; }
int fake_pyramid_shape(int i) { return g_shape[i]; }
int fake_pyramid_extent(int i) { return g_extents[i]; }
const void* fake_pyramid_label(void) { return g_label; }
void* fake_pyramid_dst(int i) { return g_dst[i]; }

int msk_label_pyramid(void* ctx, const int32_t* label, int n, int d, int h, int w, int levels, const int32_t* extents,
                      int32_t* const* dst) {
  (void)ctx;
  if (levels < 1 || levels > 8) return -1;
  ++g_calls;
  g_label = label;
  g_shape[0] = n; g_shape[1] = d; g_shape[2] = h; g_shape[3] = w;
  g_levels = levels;
  for (int i = 0; i < 3 * levels; ++i) g_extents[i] = extents[i];
  for (int i = 0; i < levels; ++i) g_dst[i] = dst[i];
  return 0;
}
