// Packed-weight cache over a row table (msk_pack_rows.h): what the Winograd cache (msk_conv_wbf.hip) and the cache of the other
// convolution kernels (msk_conv.hip) do alike.  ONE policy:
//   * a row is created at the first use of its key; its image is a device allocation of its own;
//   * with every row taken, the least recently used row is evicted; an evicted row and a row whose weights were freed are
//     DROPPED: both streams are synchronised (nothing can still read the image after that), the image is freed, and the next
//     tenant gets a fresh allocation.  Evictions need more live weight tensors than rows, frees happen at teardown: neither
//     is on the training step;
//   * rows go stale through msk_weights_changed_impl and are rebuilt TOGETHER by the optimizer kernels (msk_prepack_impl: the
//     rows used since the previous full rebuild; msk_prepack_range_impl: those inside a slice, on the optimizer's stream), or
//     alone at their next use.
// A cache supplies its device descriptor table (store) and its pack kernels (build).
#pragma once
#include "msk_common.h"
#include "msk_pack_rows.h"

template <class Desc, int N>
struct PackCache : msk_pack_cache {
  static constexpr int kRows = N;
  PackRows<Desc, N> rows;

  // pack the listed rows on the current stream and mark them valid
  virtual int build(msk_ctx* ctx, const std::vector<int>& which) = 0;
  // a new row has its image: complete its descriptor and send it to the device table (stream order; checked by row_of)
  virtual void store(msk_ctx* ctx, int r, void* image) = 0;

  // the row of key, created on first use with an image of `bytes` bytes; < 0 on error (error set)
  int row_of(msk_ctx* ctx, const Desc& key, size_t bytes) {
    int r = rows.find(key);
    if (r >= 0) {
      rows.touch(r);
      return r;
    }
    void* image = nullptr;
    r = rows.claim(key, &image);
    drop(ctx, image);
    if (hipMalloc(&image, bytes) != hipSuccess) {
      rows.release(r);
      msk_fail(ctx, __FILE__, __LINE__, "PackCache::row_of", "hipMalloc failed");
      return -1;
    }
    store(ctx, r, image);
    if (hipGetLastError() != hipSuccess) {
      drop(ctx, image);
      rows.release(r);
      msk_fail(ctx, __FILE__, __LINE__, "PackCache::row_of", "kernel launch");
      return -1;
    }
    return r;
  }

  void changed(const void* p, size_t bytes) override { rows.invalidate(p, bytes); }
  void freed(msk_ctx* ctx, const void* p, size_t bytes) override {
    // dropped, not just invalidated: the next optimizer call would rebuild the row from freed memory
    rows.drop_freed(p, bytes, [&](const Desc& d) { drop(ctx, d.image()); });
  }
  int prepack(msk_ctx* ctx, const void* p, size_t bytes) override {
    const std::vector<int> which = rows.stale_in_use(p, bytes);
    if (!p) rows.advance_epoch();
    return which.empty() ? 0 : build(ctx, which);
  }
  ~PackCache() override {
    rows.for_each_live([](const Desc& d) { (void)hipFree(d.image()); });
  }

 private:
  static void drop(msk_ctx* ctx, void* image) {
    if (!image) return;
    hipStreamSynchronize(ctx->stream);
    if (ctx->side) hipStreamSynchronize(ctx->side);
    (void)hipFree(image);
  }
};
