/* The four gradient-clipping entry points (medicalseg_amd/csrc/msk_clip.hip) for the host-only STAND-IN library:
 * tests/test_clip_host.py compiles this file together with tests/fake_msegk.c into one shared object.  Like that file it
 * computes NOTHING; the workspace size is the real formula (no GPU needed for it either), the record is left as allocated,
 * and every call is counted by name so that the test can see which update an optimizer asked for. */
#include <stddef.h>

static long g_coef = 0, g_sgd_clip = 0, g_adam_clip = 0;

long fake_clip_calls(int which) { return which == 0 ? g_coef : which == 1 ? g_sgd_clip : g_adam_clip; }

int msk_grad_clip_workspace(size_t count, size_t* bytes) {
  if (!bytes || count < 1 || count > (size_t)0x7fffffff) return -1;
  *bytes = (count + 4095) / 4096 * 8;
  return 0;
}
int msk_grad_clip_coef() { ++g_coef; return 0; }
int msk_sgd_momentum_clip() { ++g_sgd_clip; return 0; }
int msk_adam_clip() { ++g_adam_clip; return 0; }
