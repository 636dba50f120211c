// Row table of a packed-weight cache: the host bookkeeping that the Winograd cache (msk_conv_wbf.hip) and the cache of the
// other convolution kernels (msk_conv.hip) share.  Plain C++: no HIP call is made here -- whoever is handed an evicted or a
// dropped row synchronises and frees its image (msk_pack.h), so tests/pack_rows_main.cpp runs this file under sanitizers.
//
// A row belongs to one key = (weight pointer, layout).  It is LIVE while it has a tenant, VALID while its image matches the
// weights, and IN USE when it was asked for in the current or the previous epoch (an epoch ends with every full rebuild).
//
// Desc supplies:  const void* weights() const;      the canonical weight tensor ...
//                 size_t weight_bytes() const;      ... and its span in bytes
//                 void* image() const;              the packed image (nullptr: none yet)
//                 bool same_key(const Desc&) const;
#pragma once
#include <cstddef>
#include <vector>

template <class Desc, int N>
struct PackRows {
  static constexpr int kRows = N;
  struct Row {
    Desc d{};
    bool live = false, valid = false;
    long last_use = 0;
  };
  Row e[N];
  long epoch = 1;

  int find(const Desc& key) const {
    for (int r = 0; r < N; ++r)
      if (e[r].live && e[r].d.same_key(key)) return r;
    return -1;
  }
  // a row for a key that find() does not know: the first free row, else the least recently used one, whose image is reported
  // through *evicted (nullptr: nothing to release).  The row comes back live, stale and touched, its descriptor = key.
  int claim(const Desc& key, void** evicted) {
    int row = 0;
    for (int r = 0; r < N; ++r) {
      if (!e[r].live) {
        row = r;
        break;
      }
      if (e[r].last_use < e[row].last_use) row = r;
    }
    *evicted = e[row].live ? e[row].d.image() : nullptr;
    e[row] = Row();
    e[row].d = key;
    e[row].live = true;
    e[row].last_use = epoch;
    return row;
  }
  void touch(int r) { e[r].last_use = epoch; }
  void release(int r) { e[r] = Row(); }

  // [p, p + bytes) was written: the rows whose weights overlap it are stale
  void invalidate(const void* p, size_t bytes) {
    for (Row& w : e)
      if (w.live && overlaps(w.d, p, bytes)) w.valid = false;
  }
  // [p, p + bytes) was freed: the rows whose weights overlap it go to drop(const Desc&) and are released
  // (bytes == 0, range unknown: the rows whose weights begin at p)
  template <class F>
  void drop_freed(const void* p, size_t bytes, F&& drop) {
    for (Row& w : e) {
      if (!w.live || !(bytes ? overlaps(w.d, p, bytes) : w.d.weights() == p)) continue;
      drop(w.d);
      w = Row();
    }
  }
  // the stale rows in use: all of them (p == nullptr), or those whose weights lie wholly inside [p, p + bytes) -- a row that
  // straddles a slice waits for the full rebuild
  std::vector<int> stale_in_use(const void* p = nullptr, size_t bytes = 0) const {
    std::vector<int> rows;
    for (int r = 0; r < N; ++r) {
      const Row& w = e[r];
      if (!w.live || w.valid || w.last_use < epoch - 1) continue;
      const char* b0 = (const char*)w.d.weights();
      if (p && !(b0 >= (const char*)p && b0 + w.d.weight_bytes() <= (const char*)p + bytes)) continue;
      rows.push_back(r);
    }
    return rows;
  }
  void advance_epoch() { epoch += 1; }
  template <class F>
  void for_each_live(F&& f) const {
    for (const Row& w : e)
      if (w.live) f(w.d);
  }

 private:
  static bool overlaps(const Desc& d, const void* p, size_t bytes) {
    const char* a0 = (const char*)p;
    const char* b0 = (const char*)d.weights();
    return a0 < b0 + d.weight_bytes() && b0 < a0 + bytes;
  }
};
