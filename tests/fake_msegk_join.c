/* Linked with tests/fake_msegk.c by tests/test_tk_join_bookkeeping.py: the one entry point that stand-in does not have, with an
 * answer the test chooses (0 = the join backward was taken along, 1 = declined) and a call counter.  Computes nothing. */
static int g_join_rc = 0;
static long g_join_calls = 0;
void fake_join_set_rc(int rc) { g_join_rc = rc; g_join_calls = 0; }
long fake_join_calls(void) { return g_join_calls; }
int msk_conv3d_bwd_bnact_join() { ++g_join_calls; return g_join_rc; }
