// Host test of the packed-weight caches' row table (medicalseg_amd/csrc/msk_pack_rows.h) with a toy descriptor, capacity 4.
// Built and run by tests/test_pack_rows.py with -fsanitize=address,undefined; exit status 0 = every case passed.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "msk_pack_rows.h"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

namespace {

struct Toy {
  const char* w = nullptr;   // weights: n bytes at w
  size_t n = 0;
  int layout = 0, dir = 0;
  void* out = nullptr;
  const void* weights() const { return w; }
  size_t weight_bytes() const { return n; }
  void* image() const { return out; }
  bool same_key(const Toy& o) const { return w == o.w && n == o.n && layout == o.layout && dir == o.dir; }
};
using Rows = PackRows<Toy, 4>;

char g_mem[1024];      // the "device memory" the weights live in (addresses only)
char g_img[16];        // image pointers (addresses only)

Toy key(int off, size_t n = 16, int layout = 0, int dir = 0) {
  Toy t;
  t.w = g_mem + off; t.n = n; t.layout = layout; t.dir = dir;
  return t;
}
// claim a row for a key and give it image number `img`, as a cache does after its allocation
int add(Rows& t, const Toy& k, int img, void** evicted = nullptr) {
  void* ev = nullptr;
  const int r = t.claim(k, &ev);
  t.e[r].d.out = g_img + img;
  if (evicted) *evicted = ev;
  return r;
}
std::vector<int> live_rows(const Rows& t) {
  std::vector<int> v;
  for (int r = 0; r < Rows::kRows; ++r)
    if (t.e[r].live) v.push_back(r);
  return v;
}

void test_find() {
  Rows t;
  CHECK(t.find(key(0)) < 0);
  const int r = add(t, key(0, 16, 1, 1), 0);
  CHECK(t.e[r].live && !t.e[r].valid && t.e[r].last_use == t.epoch);
  CHECK(t.find(key(0, 16, 1, 1)) == r);
  CHECK(t.find(key(4, 16, 1, 1)) < 0);    // each field of the key on its own
  CHECK(t.find(key(0, 12, 1, 1)) < 0);
  CHECK(t.find(key(0, 16, 2, 1)) < 0);
  CHECK(t.find(key(0, 16, 1, 0)) < 0);
}

void test_claim_free_then_lru() {
  Rows t;
  void* ev = g_img;
  int rows[4];
  for (int i = 0; i < 4; ++i) {
    rows[i] = add(t, key(100 * i), i, &ev);
    CHECK(ev == nullptr);                  // a free row has nothing to release
    t.advance_epoch();                     // row i was last used in epoch 1 + i
  }
  CHECK(std::set<int>(rows, rows + 4).size() == 4);
  t.release(rows[2]);                      // a free row is preferred to any live one ...
  CHECK(add(t, key(500), 5, &ev) == rows[2] && ev == nullptr);
  t.touch(rows[0]);                        // ... touching protects the oldest row ...
  const int r = add(t, key(600), 6, &ev);  // ... so the second oldest is the victim, and its image is reported
  CHECK(r == rows[1] && ev == g_img + 1);
  CHECK(t.find(key(100)) < 0 && t.find(key(600)) == r && t.find(key(0)) == rows[0]);
  CHECK(!t.e[r].valid && t.e[r].d.out == g_img + 6);
  CHECK(live_rows(t).size() == 4);
}

void test_invalidate() {
  // rows at [100, 116), [200, 216), [300, 316)
  auto fresh = [](Rows& t, int r[3]) {
    for (int i = 0; i < 3; ++i) {
      r[i] = add(t, key(100 * (i + 1)), i);
      t.e[r[i]].valid = true;
    }
  };
  int r[3];
  {
    Rows t;
    fresh(t, r);
    t.invalidate(g_mem + 90, 11);          // overlaps the first byte of row 0
    CHECK(!t.e[r[0]].valid && t.e[r[1]].valid && t.e[r[2]].valid);
  }
  {
    Rows t;
    fresh(t, r);
    t.invalidate(g_mem + 215, 50);         // overlaps the last byte of row 1
    CHECK(t.e[r[0]].valid && !t.e[r[1]].valid && t.e[r[2]].valid);
  }
  {
    Rows t;
    fresh(t, r);
    t.invalidate(g_mem + 304, 4);          // inside row 2
    CHECK(t.e[r[0]].valid && t.e[r[1]].valid && !t.e[r[2]].valid);
    t.e[r[2]].valid = true;
    t.invalidate(g_mem + 150, 400);        // contains rows 1 and 2
    CHECK(t.e[r[0]].valid && !t.e[r[1]].valid && !t.e[r[2]].valid);
  }
  {
    Rows t;
    fresh(t, r);
    t.invalidate(g_mem + 116, 84);         // [116, 200): touches the end of row 0 and the start of row 1, overlaps neither
    t.invalidate(g_mem + 84, 16);          // [84, 100): a1 == b0
    CHECK(t.e[r[0]].valid && t.e[r[1]].valid && t.e[r[2]].valid);
  }
}

void test_freed() {
  std::vector<void*> dropped;
  auto drop = [&](const Toy& d) { dropped.push_back(d.out); };
  {
    // bytes == 0: only the rows whose weights BEGIN at p (two layouts of one tensor), not one that merely contains p
    Rows t;
    const int a = add(t, key(100, 16, 0), 0), b = add(t, key(100, 16, 1), 1), c = add(t, key(96, 16), 2), d = add(t, key(200), 3);
    t.drop_freed(g_mem + 100, 0, drop);
    CHECK(dropped.size() == 2 && std::set<void*>(dropped.begin(), dropped.end()) == (std::set<void*>{g_img + 0, g_img + 1}));
    CHECK(!t.e[a].live && !t.e[b].live && t.e[c].live && t.e[d].live);
    CHECK(t.find(key(100, 16, 0)) < 0 && t.find(key(100, 16, 1)) < 0 && t.find(key(96, 16)) == c);
  }
  dropped.clear();
  {
    // a range: every overlapping row, each seen once
    Rows t;
    const int a = add(t, key(100), 0), b = add(t, key(200), 1), c = add(t, key(300), 2), d = add(t, key(400), 3);
    t.drop_freed(g_mem + 110, 195, drop);  // [110, 305): partly row a, all of b, the head of c
    CHECK(dropped.size() == 3 && std::set<void*>(dropped.begin(), dropped.end()) == (std::set<void*>{g_img + 0, g_img + 1, g_img + 2}));
    CHECK(!t.e[a].live && !t.e[b].live && !t.e[c].live && t.e[d].live);
    CHECK(t.find(key(100)) < 0 && t.find(key(200)) < 0 && t.find(key(300)) < 0 && t.find(key(400)) == d);
    void* ev = g_img;
    CHECK(add(t, key(500), 5, &ev) == a && ev == nullptr);   // a dropped row is a free row again
  }
}

void test_collect() {
  Rows t;
  const int a = add(t, key(100), 0);       // epoch 1
  t.advance_epoch();
  const int b = add(t, key(200), 1);       // epoch 2
  t.advance_epoch();
  const int c = add(t, key(300), 2);       // epoch 3 = current
  const int d = add(t, key(400), 3);
  t.e[d].valid = true;
  // stale rows used in the current (c) or the previous (b) epoch; a was used earlier, d is valid
  CHECK(t.stale_in_use() == (std::vector<int>{b, c}));
  CHECK(t.epoch == 3);
  CHECK(t.find(key(100)) == a && !t.e[a].valid);   // the row left out is still reported stale at its next lookup
  // the slice form: rows wholly inside [p, p + bytes) only, and the epoch stays
  CHECK(t.stale_in_use(g_mem + 200, 116) == (std::vector<int>{b, c}));   // [200, 316)
  CHECK(t.stale_in_use(g_mem + 200, 115) == (std::vector<int>{b}));      // c straddles the end
  CHECK(t.stale_in_use(g_mem + 201, 115) == (std::vector<int>{c}));      // b straddles the start
  CHECK(t.stale_in_use(g_mem + 0, 1000) == (std::vector<int>{b, c}));    // a is inside, but not in use
  CHECK(t.epoch == 3);
  t.touch(a);
  CHECK(t.stale_in_use() == (std::vector<int>{a, b, c}));
  t.advance_epoch();
  t.advance_epoch();
  CHECK(t.stale_in_use().empty());
}

void test_teardown() {
  Rows t;
  int n = 0;
  t.for_each_live([&](const Toy&) { ++n; });
  CHECK(n == 0);
  add(t, key(100), 0);
  const int b = add(t, key(200), 1);
  add(t, key(300), 2);
  t.release(b);
  std::set<void*> seen;
  t.for_each_live([&](const Toy& d) { CHECK(seen.insert(d.out).second); });
  CHECK(seen == (std::set<void*>{g_img + 0, g_img + 2}));
}

}  // namespace

int main() {
  test_find();
  test_claim_free_then_lru();
  test_invalidate();
  test_freed();
  test_collect();
  test_teardown();
  std::printf("pack_rows: all cases passed\n");
  return 0;
}
