// Connected-component labelling of binary masks on gfx950: the device path of the reference's
// BinaryMaskToConnectComponent / TopkLargestConnectComponent (transforms/functional.py:117-131,
// transform.py:343-396).  The host restatement medicalseg_amd/transforms/transform.py::_connected_components is the
// specification: 6-connected foreground (value != 0) components numbered 1, 2, ... by decreasing size, ties by the
// component's first voxel in raster order, components below `minimum_volume` dropped (0) and the later ranks closed
// up, ranks above k dropped when k > 0.  Every volume of the batch is labelled on its own.
//
// Passes (all integer atomics: the labels are deterministic whatever the schedule):
//   init      min / max word per volume (binary check), status / count words
//   local     one workgroup per 4 x 8 x 32 tile: union-find in LDS, every voxel points at its tile-local root
//             (global linear index); one min / max atomic pair per tile
//   merge     union across the tiles' low faces with global atomicMin, larger root linked under the smaller:
//             a root is its component's MINIMUM linear index = its first voxel in raster order
//   flatten   (new launch: the links are final) every voxel -> its root; sizes summed per tile in an LDS hash, one
//             global atomicAdd per (tile, root); the binary check against the volume's min / max
//   compact   the roots in ascending index order (stable one-bit split)
//   sort      LSD radix sort, 8-bit digits, of the key (volume, V - size): stable, so equal sizes keep the
//             ascending root order of the compaction
//   rank      segment starts per volume, then rank -> kept label per root; relabel every voxel
//
// Scratch (msk_workspace): T + 2 M + max(256 ceil(M / 8192), 2 ceil(T / 8192)) + 3 n + 64 int32 words with T = n d h w
// voxels and M = n ceil(d h w / 2) (a 6-connected volume holds at most ceil(V/2) components: the checkerboard), i.e.
// about 2.02 words per voxel plus 3 per volume.
//
// Status word per volume (caller-owned, written by the device; no host synchronisation inside the call):
//   bit 0 -- the volume holds 3 or more distinct values (the reference's binary assert);
//   bit 1 -- a find / union loop hit its iteration bound (a bug, not an input property: the labels are garbage).
//
// msk_fill_holes3d (at the end of the file) runs the local and merge passes on the ZERO voxels instead, with the links in
// scratch, and follows them with a gather of three words per root and an elementwise apply: no compaction, sort or rank.
#include <algorithm>
#include <climits>
#include <type_traits>

#include "msk_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTD = 4, kTH = 8, kTW = 32;   // tile: 1024 voxels, 4 per thread, 128-byte rows along w
constexpr int kTile = kTD * kTH * kTW;
constexpr int kHash = 2 * kTile;            // LDS hash of the flatten pass: load factor <= 1/2
constexpr int kChunk = 8192;                // items per radix workgroup
constexpr int kIpt = kChunk / kThreads;     // 32 per thread, held in registers
constexpr int kStatusNonBinary = 1, kStatusBound = 2;

struct Geo {
  int d, h, w;
  int tz, ty, tx;    // tiles per axis
  long vv;           // voxels per volume
};

__device__ __forceinline__ int ld_agent(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_lds(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// float bits -> int with the float order (-0.0 folded onto +0.0: np.unique sees one zero); int32 as is
template <typename T>
__device__ __forceinline__ int order_key(T v) {
  if constexpr (std::is_same<T, float>::value) {
    const float f = (float)v == 0.f ? 0.f : (float)v;
    const int b = __float_as_int(f);
    return b < 0 ? b ^ 0x7fffffff : b;
  } else {
    return (int)v;
  }
}

__global__ void ccl_init_k(int* __restrict__ mm, int* __restrict__ status, int* __restrict__ counts, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (mm) {   // hole filling has no binary check
      mm[2 * i] = INT_MAX;
      mm[2 * i + 1] = INT_MIN;
    }
    status[i] = 0;
    if (counts) counts[i] = 0;
  }
}

__device__ __forceinline__ void tile_coords(const Geo& g, int blk, int& vol, int& z0, int& y0, int& x0) {
  const int per = g.tz * g.ty * g.tx;
  vol = blk / per;
  int t = blk - vol * per;
  const int bz = t / (g.ty * g.tx);
  t -= bz * g.ty * g.tx;
  const int by = t / g.tx, bx = t - by * g.tx;
  z0 = bz * kTD;
  y0 = by * kTH;
  x0 = bx * kTW;
}

// ---- local: LDS union-find on one tile ------------------------------------------------------------------------
// lp[l] = -1 (background) or a tile-local index <= l.  Local indices follow the raster order of the tile, which is
// the order of the global indices, so the tile-local minimum is also the global minimum of the piece.
__device__ __forceinline__ int lds_find(int* lp, int a, bool& bad) {
  for (int it = 0; it < kTile; ++it) {
    const int p = ld_lds(&lp[a]);
    if (p == a) return a;
    a = p;
  }
  bad = true;
  return a;
}

__device__ __forceinline__ void lds_union(int* lp, int a, int b, bool& bad) {
  // max(find(a), find(b)) strictly decreases every round: at most kTile rounds
  for (int it = 0; it < kTile; ++it) {
    a = lds_find(lp, a, bad);
    b = lds_find(lp, b, bad);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&lp[a], b);
    if (old == a) return;
    a = old;
  }
  bad = true;
}

// FILL == 0: the members are the voxels != 0 and sizes[] is cleared (connected components).  FILL == 1 | 3 (hole filling):
// the members are the voxels == 0 (-0.0 is one, a NaN is not), `sizes` holds FILL words per voxel that are initialised at
// the tile-local roots only -- {border flag = 0}, then {smallest, largest enclosing value} = {INT_MAX, INT_MIN} -- and mm is
// not used.
template <typename T, int FILL>
__global__ void __launch_bounds__(kThreads)
ccl_local_k(const T* __restrict__ src, int* __restrict__ par, int* __restrict__ sizes, int* __restrict__ mm,
            int* __restrict__ status, Geo g) {
  __shared__ int lp[kTile];
  __shared__ int smin[kThreads / 64], smax[kThreads / 64];
  int vol, z0, y0, x0;
  tile_coords(g, blockIdx.x, vol, z0, y0, x0);
  const size_t vbase = (size_t)vol * g.vv;
  const int tid = threadIdx.x, y = tid / kTW, x = tid % kTW;
  int lo = INT_MAX, hi = INT_MIN;
#pragma unroll
  for (int z = 0; z < kTD; ++z) {
    const int l = (z * kTH + y) * kTW + x;
    const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
    int v = -1;
    if (gz < g.d && gy < g.h && gx < g.w) {
      const T s = src[vbase + ((size_t)gz * g.h + gy) * g.w + gx];
      const int key = order_key(s);
      lo = min(lo, key);
      hi = max(hi, key);
      if (FILL ? s == (T)0 : s != (T)0) v = l;
    }
    lp[l] = v;
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_down(lo, o, 64));
    hi = max(hi, __shfl_down(hi, o, 64));
  }
  if (tid % 64 == 0) {
    smin[tid / 64] = lo;
    smax[tid / 64] = hi;
  }
  __syncthreads();
  bool bad = false;
#pragma unroll
  for (int z = 0; z < kTD; ++z) {
    const int l = (z * kTH + y) * kTW + x;
    if (ld_lds(&lp[l]) < 0) continue;   // background stays -1; a foreground entry only ever decreases, never to -1
    if (x > 0 && ld_lds(&lp[l - 1]) >= 0) lds_union(lp, l, l - 1, bad);
    if (y > 0 && ld_lds(&lp[l - kTW]) >= 0) lds_union(lp, l, l - kTW, bad);
    if (z > 0 && ld_lds(&lp[l - kTH * kTW]) >= 0) lds_union(lp, l, l - kTH * kTW, bad);
  }
  __syncthreads();
#pragma unroll
  for (int z = 0; z < kTD; ++z) {
    const int l = (z * kTH + y) * kTW + x;
    const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
    if (gz < g.d && gy < g.h && gx < g.w) {
      const size_t gi = vbase + ((size_t)gz * g.h + gy) * g.w + gx;
      int out = -1;
      if (lp[l] >= 0) {
        const int r = lds_find(lp, l, bad);
        const int rz = r / (kTH * kTW), ry = (r / kTW) % kTH, rx = r % kTW;
        out = (int)(vbase + ((size_t)(z0 + rz) * g.h + (y0 + ry)) * g.w + (x0 + rx));
      }
      par[gi] = out;
      if constexpr (FILL == 0) {
        sizes[gi] = 0;
      } else if (out == (int)gi) {   // a root of the merged forest is a root here: the words of the others are never read
        sizes[FILL * gi] = 0;
        if constexpr (FILL == 3) {
          sizes[3 * gi + 1] = INT_MAX;
          sizes[3 * gi + 2] = INT_MIN;
        }
      }
    }
  }
  if (bad) atomicOr(&status[vol], kStatusBound);
  if (FILL == 0 && tid == 0) {
    for (int w = 1; w < kThreads / 64; ++w) {   // lane 0 of wavefront 0 already holds its own wavefront's
      lo = min(lo, smin[w]);
      hi = max(hi, smax[w]);
    }
    // every tile of a volume targets the same two words (Guideline 12): most tiles of a binary mask bring nothing new,
    // and a stale read can only be OLDER = a larger min / smaller max, i.e. cost an atomic that was not needed
    if (lo < ld_agent(&mm[2 * vol])) atomicMin(&mm[2 * vol], lo);
    if (hi > ld_agent(&mm[2 * vol + 1])) atomicMax(&mm[2 * vol + 1], hi);
  }
}

// ---- merge: union across tile faces ---------------------------------------------------------------------------
// par[] only ever DECREASES (atomicMin), and every value it takes is a member of the same component that is <= the
// entry's index.  Other workgroups' atomicMin results may be invisible to a plain load here (the XCDs' L2s are not
// coherent), so every read of a link is an agent-scope atomic load; even so a read may return an OLDER link.  An
// older link is still a valid ancestor: find() then walks one hop more, and a root that is no longer a root makes
// the atomicMin return a value != the root, so union() retries from that value.  A stale read costs a retry, never a
// wrong label.  Path halving (atomicMin of the grand-parent) keeps the chains short and keeps the monotone invariant.
__device__ __forceinline__ int g_find(int* par, int a, long bound, bool& bad) {
  int p = ld_agent(&par[a]);
  for (long it = 0; it < bound; ++it) {
    if (p == a) return a;
    const int gp = ld_agent(&par[p]);
    if (gp != p) atomicMin(&par[a], gp);
    a = p;
    p = gp;
  }
  bad = true;
  return a;
}

__device__ __forceinline__ void g_union(int* par, int a, int b, long bound, bool& bad) {
  for (long it = 0; it < bound; ++it) {   // max(find(a), find(b)) strictly decreases every round
    a = g_find(par, a, bound, bad);
    b = g_find(par, b, bound, bad);
    if (a == b || bad) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&par[a], b);
    if (old == a) return;
    a = old;
  }
  bad = true;
}

__global__ void __launch_bounds__(kThreads)
ccl_merge_k(int* __restrict__ par, int* __restrict__ status, Geo g, long total) {
  const long hw = (long)g.h * g.w;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long vol = i / g.vv, r = i - vol * g.vv;
    const int z = (int)(r / hw), y = (int)((r / g.w) % g.h), x = (int)(r % g.w);
    const bool fx = x > 0 && x % kTW == 0, fy = y > 0 && y % kTH == 0, fz = z > 0 && z % kTD == 0;
    if (!(fx || fy || fz)) continue;
    // foreground-ness (>= 0) was fixed by the previous launch and never changes: a plain load is exact for it
    if (par[i] < 0) continue;
    bool bad = false;
    const long bound = g.vv + 1;   // indices strictly decrease along a chain inside one volume
    if (fx && par[i - 1] >= 0) g_union(par, (int)i, (int)(i - 1), bound, bad);
    if (fy && par[i - g.w] >= 0) g_union(par, (int)i, (int)(i - g.w), bound, bad);
    if (fz && par[i - hw] >= 0) g_union(par, (int)i, (int)(i - hw), bound, bad);
    if (bad) atomicOr(&status[vol], kStatusBound);
  }
}

// ---- flatten + sizes + binary check ---------------------------------------------------------------------------
// A new launch: every link written by the merge is visible.  Writing a root into par[] while other workgroups walk
// it is safe: they read either the old link or the root, both ancestors.
template <typename T>
__global__ void __launch_bounds__(kThreads)
ccl_flatten_k(const T* __restrict__ src, int* __restrict__ par, int* __restrict__ sizes, const int* __restrict__ mm,
              int* __restrict__ status, Geo g) {
  __shared__ int hkey[kHash], hcnt[kHash];
  for (int i = threadIdx.x; i < kHash; i += kThreads) {
    hkey[i] = -1;
    hcnt[i] = 0;
  }
  __syncthreads();
  int vol, z0, y0, x0;
  tile_coords(g, blockIdx.x, vol, z0, y0, x0);
  const size_t vbase = (size_t)vol * g.vv;
  const int lo = mm[2 * vol], hi = mm[2 * vol + 1];
  const int tid = threadIdx.x, y = tid / kTW, x = tid % kTW;
  bool bad = false, nonbin = false;
#pragma unroll
  for (int z = 0; z < kTD; ++z) {
    const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
    if (!(gz < g.d && gy < g.h && gx < g.w)) continue;
    const size_t gi = vbase + ((size_t)gz * g.h + gy) * g.w + gx;
    const int key = order_key(src[gi]);
    nonbin |= key != lo && key != hi;
    int a = par[gi];
    if (a < 0) continue;
    int p = par[a];
    for (long it = 0; p != a; ++it) {
      if (it > g.vv) { bad = true; break; }
      a = p;
      p = par[a];
    }
    par[gi] = a;
    // LDS hash: linear probing from a mixed slot; at most kTile distinct keys in a table of 2 kTile slots
    unsigned s = ((unsigned)a * 2654435761u) % kHash;
    for (int probe = 0; probe < kHash; ++probe) {
      const int k = atomicCAS(&hkey[s], -1, a);
      if (k == -1 || k == a) {
        atomicAdd(&hcnt[s], 1);
        break;
      }
      s = s + 1 == kHash ? 0 : s + 1;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kHash; i += kThreads) {
    const int k = hkey[i];
    if (k >= 0) atomicAdd(&sizes[k], hcnt[i]);
  }
  if (bad) atomicOr(&status[vol], kStatusBound);
  if (nonbin) atomicOr(&status[vol], kStatusNonBinary);
}

// ---- stable counting passes (compaction and radix sort) -------------------------------------------------------
// MODE 0: items are the voxel indices 0..count-1, digit 0 = "is a root" (par[i] == i), only digit 0 is stored.
// MODE 1: items are roots from `in`, digit = byte `shift / 8` of ((vol << sbits) | (vv - size)).
// hist[digit * nb + block] (nb = the number of ACTIVE blocks, derived from the item count on the device).
template <int MODE>
__device__ __forceinline__ int item_digit(int item, const int* __restrict__ aux, long vv, int sbits, int shift) {
  if constexpr (MODE == 0) {
    return aux[item] == item ? 0 : 1;
  } else {
    const unsigned long long vol = (unsigned long long)(item / vv);
    const unsigned long long key = (vol << sbits) | (unsigned long long)(vv - aux[item]);
    return (int)((key >> shift) & 255);
  }
}

__device__ __forceinline__ int item_count(const int* cnt_dev, int cnt_host) { return cnt_dev ? *cnt_dev : cnt_host; }

// A thread's kIpt items and their digits are loaded before any of them is used: the gathers (in[], then sizes[] of a
// random root) of all rounds are in flight together instead of one memory latency per round.
template <int MODE>
__device__ __forceinline__ void load_items(const int* __restrict__ in, const int* __restrict__ aux, int beg, int end,
                                           long vv, int sbits, int shift, int (&item)[kIpt], int (&dg)[kIpt]) {
#pragma unroll
  for (int r = 0; r < kIpt; ++r) {
    const int i = beg + r * kThreads + (int)threadIdx.x;
    item[r] = i < end ? (MODE == 0 ? i : in[i]) : -1;
  }
#pragma unroll
  for (int r = 0; r < kIpt; ++r) dg[r] = item[r] >= 0 ? item_digit<MODE>(item[r], aux, vv, sbits, shift) : 0;
}

template <int MODE>
__global__ void __launch_bounds__(kThreads)
ccl_hist_k(const int* __restrict__ in, const int* __restrict__ aux, const int* __restrict__ cnt_dev, int cnt_host, long vv,
           int sbits, int shift, int* __restrict__ hist) {
  constexpr int ND = MODE == 0 ? 2 : 256;
  __shared__ int h[ND];
  const int count = item_count(cnt_dev, cnt_host);
  const int nb = (count + kChunk - 1) / kChunk;
  if ((int)blockIdx.x >= nb) return;
  for (int i = threadIdx.x; i < ND; i += kThreads) h[i] = 0;
  const int beg = blockIdx.x * kChunk, end = min(count, beg + kChunk);
  int item[kIpt], dg[kIpt];
  load_items<MODE>(in, aux, beg, end, vv, sbits, shift, item, dg);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kIpt; ++r)
    if (item[r] >= 0) atomicAdd(&h[dg[r]], 1);
  __syncthreads();
  for (int i = threadIdx.x; i < ND; i += kThreads) hist[i * nb + blockIdx.x] = h[i];
}

// exclusive scan of hist[0 .. ND * nb) in one workgroup of 1024 threads, 4 entries per thread per round;
// MODE 0 also stores the number of digit-0 items (the roots) into *nout, clamped to the root buffers' `cap`
template <int MODE>
__global__ void __launch_bounds__(1024)
ccl_scan_k(int* __restrict__ hist, const int* __restrict__ cnt_dev, int cnt_host, int* __restrict__ nout, int cap) {
  constexpr int ND = MODE == 0 ? 2 : 256;
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int count = item_count(cnt_dev, cnt_host);
  const int nb = (count + kChunk - 1) / kChunk;
  const int total = ND * nb;
  const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < total; base += 4096) {
    int v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = base + tid * 4 + j;
      v[j] = i < total ? hist[i] : 0;
      s += v[j];
    }
    int inc = s;   // inclusive wave scan
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = carry_s;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    int run = before + inc - s;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = base + tid * 4 + j;
      if (i < total) hist[i] = run;
      run += v[j];
    }
    __syncthreads();
    if (tid == 1023) carry_s = run;
    __syncthreads();
  }
  if (MODE == 0 && tid == 0) *nout = min(nb > 0 ? hist[nb] : 0, cap);   // start of digit 1 = number of digit-0 items
}

// stable scatter: rounds of 256 items in order; a lane's place among equal digits of its wavefront comes from eight
// ballots, the wavefronts before it from LDS counts, the rounds before it from a running offset per digit
template <int MODE>
__global__ void __launch_bounds__(kThreads)
ccl_scatter_k(const int* __restrict__ in, const int* __restrict__ aux, const int* __restrict__ cnt_dev, int cnt_host,
              long vv, int sbits, int shift, const int* __restrict__ hist, int* __restrict__ out, int cap) {
  constexpr int ND = MODE == 0 ? 2 : 256;
  constexpr int NBITS = MODE == 0 ? 1 : 8;
  constexpr int NW = kThreads / 64;
  __shared__ int run[ND];
  __shared__ int wcnt[NW][ND];
  const int count = item_count(cnt_dev, cnt_host);
  const int nb = (count + kChunk - 1) / kChunk;
  if ((int)blockIdx.x >= nb) return;
  const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64;
  for (int i = tid; i < ND; i += kThreads) run[i] = hist[i * nb + blockIdx.x];
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int beg = blockIdx.x * kChunk, end = min(count, beg + kChunk);
  int items[kIpt], dgs[kIpt];
  load_items<MODE>(in, aux, beg, end, vv, sbits, shift, items, dgs);
#pragma unroll
  for (int r = 0; r < kIpt; ++r) {
    if (beg + r * kThreads >= end) break;   // uniform over the workgroup
    for (int i = tid; i < NW * ND; i += kThreads) (&wcnt[0][0])[i] = 0;
    __syncthreads();
    const int item = items[r], dg = dgs[r];
    const bool valid = item >= 0;
    unsigned long long match = __ballot(valid);
#pragma unroll
    for (int b = 0; b < NBITS; ++b) {
      const unsigned long long bb = __ballot((dg >> b) & 1);
      match &= ((dg >> b) & 1) ? bb : ~bb;
    }
    const int pre = __popcll(match & lt);
    if (valid && pre == 0) wcnt[wave][dg] = __popcll(match);
    __syncthreads();
    if (valid && (MODE == 1 || dg == 0)) {
      int pos = run[dg] + pre;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][dg];
      if (pos < cap) out[pos] = item;   // always true for a correct labelling (at most M roots): a guard, not a case
    }
    __syncthreads();
    for (int d = tid; d < ND; d += kThreads) {
      int s = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) s += wcnt[w][d];
      run[d] += s;
    }
    __syncthreads();
  }
}

// ---- ranks ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
ccl_segstart_k(const int* __restrict__ sorted, const int* __restrict__ nroots, long vv, int* __restrict__ seg) {
  const int count = *nroots;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < count; j += gridDim.x * blockDim.x) {
    const long vol = sorted[j] / vv;
    if (j == 0 || sorted[j - 1] / vv != vol) seg[vol] = j;
  }
}

__device__ __forceinline__ bool kept(int size, int rank, int minvol, int k) {
  return size >= minvol && (k <= 0 || rank <= k);
}

// counts[vol] = the number of kept components: kept ranks are a prefix of the volume's segment (sizes descend)
__global__ void __launch_bounds__(kThreads)
ccl_counts_k(const int* __restrict__ sorted, const int* __restrict__ nroots, long vv, const int* __restrict__ seg,
             const int* __restrict__ sizes, int minvol, int k, int* __restrict__ counts) {
  const int count = *nroots;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < count; j += gridDim.x * blockDim.x) {
    const int r = sorted[j];
    const long vol = r / vv;
    const int rank = j - seg[vol] + 1;
    if (!kept(sizes[r], rank, minvol, k)) continue;
    const bool last = j + 1 == count || sorted[j + 1] / vv != vol || !kept(sizes[sorted[j + 1]], rank + 1, minvol, k);
    if (last) counts[vol] = rank;
  }
}

// sizes[root] -> kept label (rank, or 0)
__global__ void __launch_bounds__(kThreads)
ccl_assign_k(const int* __restrict__ sorted, const int* __restrict__ nroots, long vv, const int* __restrict__ seg,
             int* __restrict__ sizes, int minvol, int k) {
  const int count = *nroots;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < count; j += gridDim.x * blockDim.x) {
    const int r = sorted[j];
    const int rank = j - seg[r / vv] + 1;
    sizes[r] = kept(sizes[r], rank, minvol, k) ? rank : 0;
  }
}

__global__ void __launch_bounds__(kThreads)
ccl_relabel_k(int* __restrict__ lab, const int* __restrict__ map, long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int r = lab[i];
    lab[i] = r >= 0 ? map[r] : 0;
  }
}

inline int bits_for(long v) {   // bits needed to hold 0..v
  int b = 0;
  while (v > 0) {
    ++b;
    v >>= 1;
  }
  return b;
}

template <typename T>
int run_ccl(msk_ctx* ctx, const T* src, int32_t* dst, int n, int d, int h, int w, int minvol, int k, int32_t* status,
            int32_t* counts) {
  Geo g;
  g.d = d;
  g.h = h;
  g.w = w;
  g.tz = (d + kTD - 1) / kTD;
  g.ty = (h + kTH - 1) / kTH;
  g.tx = (w + kTW - 1) / kTW;
  g.vv = (long)d * h * w;
  const long T_ = (long)n * g.vv;
  const long M = (long)n * ((g.vv + 1) / 2);
  const long nb_sort = (M + kChunk - 1) / kChunk, nb_comp = (T_ + kChunk - 1) / kChunk;
  const long hist_words = std::max(256 * nb_sort, 2 * nb_comp);
  const long words = T_ + 2 * M + hist_words + 3L * n + 64;
  int* ws = (int*)msk_workspace(ctx, (size_t)words * sizeof(int));
  if (!ws) return -1;
  int* sizes = ws;
  int* rootsA = sizes + T_;
  int* rootsB = rootsA + M;
  int* hist = rootsB + M;
  int* mm = hist + hist_words;
  int* seg = mm + 2L * n;
  int* nroots = seg + n;
  int* par = dst;
  const long ntiles = (long)n * g.tz * g.ty * g.tx;
  hipStream_t st = ctx->stream;
  {
    msk_launch_scope ls(ctx, "ccl_init");
    hipLaunchKernelGGL(ccl_init_k, dim3(std::max(1, std::min(64, (n + kThreads - 1) / kThreads))), dim3(kThreads), 0, st,
                       mm, status, counts, n);
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "ccl_local");
    hipLaunchKernelGGL((ccl_local_k<T, 0>), dim3((unsigned)ntiles), dim3(kThreads), 0, st, src, par, sizes, mm, status, g);
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "ccl_merge");
    hipLaunchKernelGGL(ccl_merge_k, dim3(msk_ew_blocks(T_, ctx->num_cu)), dim3(kThreads), 0, st, par, status, g, T_);
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "ccl_flatten");
    hipLaunchKernelGGL(ccl_flatten_k<T>, dim3((unsigned)ntiles), dim3(kThreads), 0, st, src, par, sizes, mm, status, g);
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "ccl_compact");
    hipLaunchKernelGGL(ccl_hist_k<0>, dim3((unsigned)nb_comp), dim3(kThreads), 0, st, (const int*)nullptr, par,
                       (const int*)nullptr, (int)T_, g.vv, 0, 0, hist);
    hipLaunchKernelGGL(ccl_scan_k<0>, dim3(1), dim3(1024), 0, st, hist, (const int*)nullptr, (int)T_, nroots, (int)M);
    hipLaunchKernelGGL(ccl_scatter_k<0>, dim3((unsigned)nb_comp), dim3(kThreads), 0, st, (const int*)nullptr, par,
                       (const int*)nullptr, (int)T_, g.vv, 0, 0, (const int*)hist, rootsA, (int)M);
    MSK_LAUNCH_CHECK(ctx);
  }
  // key = (vol << sbits) | (vv - size): vv - size lies in [0, vv - 1]
  const int sbits = bits_for(g.vv - 1), vbits = bits_for((long)n - 1);
  const int passes = std::max(1, (sbits + vbits + 7) / 8);
  int* in = rootsA;
  int* out = rootsB;
  {
    msk_launch_scope ls(ctx, "ccl_sort");
    for (int p = 0; p < passes; ++p) {
      hipLaunchKernelGGL(ccl_hist_k<1>, dim3((unsigned)nb_sort), dim3(kThreads), 0, st, (const int*)in, (const int*)sizes,
                         (const int*)nroots, 0, g.vv, sbits, 8 * p, hist);
      hipLaunchKernelGGL(ccl_scan_k<1>, dim3(1), dim3(1024), 0, st, hist, (const int*)nroots, 0, (int*)nullptr, (int)M);
      hipLaunchKernelGGL(ccl_scatter_k<1>, dim3((unsigned)nb_sort), dim3(kThreads), 0, st, (const int*)in,
                         (const int*)sizes, (const int*)nroots, 0, g.vv, sbits, 8 * p, (const int*)hist, out, (int)M);
      std::swap(in, out);
    }
    MSK_LAUNCH_CHECK(ctx);
  }
  const int nbr = msk_ew_blocks(M, ctx->num_cu);
  {
    msk_launch_scope ls(ctx, "ccl_rank");
    hipLaunchKernelGGL(ccl_segstart_k, dim3(nbr), dim3(kThreads), 0, st, (const int*)in, (const int*)nroots, g.vv, seg);
    if (counts)
      hipLaunchKernelGGL(ccl_counts_k, dim3(nbr), dim3(kThreads), 0, st, (const int*)in, (const int*)nroots, g.vv,
                         (const int*)seg, (const int*)sizes, minvol, k, counts);
    hipLaunchKernelGGL(ccl_assign_k, dim3(nbr), dim3(kThreads), 0, st, (const int*)in, (const int*)nroots, g.vv,
                       (const int*)seg, sizes, minvol, k);
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "ccl_relabel");
    hipLaunchKernelGGL(ccl_relabel_k, dim3(msk_ew_blocks(T_, ctx->num_cu)), dim3(kThreads), 0, st, par, (const int*)sizes, T_);
    MSK_LAUNCH_CHECK(ctx);
  }
  return 0;
}

// ---- hole filling ---------------------------------------------------------------------------------------------------
// The components of the ZERO voxels (ccl_local_k<T, FILL>, ccl_merge_k), then per root the words {touches a face of the
// volume (OR)} and, for the label form, {smallest, largest non-zero 6-neighbour (MIN, MAX)}; a hole is a component whose
// flag stayed 0, and the label form fills it when smallest == largest.  None of compaction, sort, rank and relabel.
constexpr int kFillMaxClasses = 64;
struct FillClasses {
  int n;
  int v[kFillMaxClasses];
};

// gather (a new launch: the links are final): every zero voxel -> its root, as in ccl_flatten_k; what the voxel brings to
// its root's words is merged per tile in an LDS hash, so a tile sends at most one atomic per (root, word), and only where
// an agent-scope load says the word still moves -- the outside component is present in almost every tile, and after the
// first few tiles nothing more is sent for it.  A stale load can only cost an atomic that was not needed (the flag only
// rises, the minimum only falls, the maximum only rises).  A voxel that brings nothing (interior of a zero region) skips
// the hash.
// A tile of 1024 voxels holds at most 512 6-connected pieces (the checkerboard), so 1024 slots keep the load factor <= 1/2;
// five tables of that size are 20 KB, which leaves room for eight workgroups per CU.
constexpr int kFillHash = kTile;
template <typename T, bool LABEL>
__global__ void __launch_bounds__(kThreads)
fill_gather_k(const T* __restrict__ src, int* __restrict__ par, int* __restrict__ words, int* __restrict__ status, Geo g) {
  constexpr int W = LABEL ? 3 : 1;
  __shared__ int hkey[kFillHash], hflag[kFillHash];
  __shared__ int hlo[LABEL ? kFillHash : 1], hhi[LABEL ? kFillHash : 1], hshared[LABEL ? kFillHash : 1];
  for (int i = threadIdx.x; i < kFillHash; i += kThreads) {
    hkey[i] = -1;
    hflag[i] = 0;
    if constexpr (LABEL) {
      hlo[i] = INT_MAX;
      hhi[i] = INT_MIN;
      hshared[i] = 0;
    }
  }
  __syncthreads();
  int vol, z0, y0, x0;
  tile_coords(g, blockIdx.x, vol, z0, y0, x0);
  const size_t vbase = (size_t)vol * g.vv;
  const long hw = (long)g.h * g.w;
  const int tid = threadIdx.x, y = tid / kTW, x = tid % kTW;
  const int lane = tid % 64;
  bool bad = false;
  // what one lane sends to the hash for root `key`
  auto insert = [&](int key, bool flag, int lo, int hi, bool crosses) {
    unsigned s = ((unsigned)key * 2654435761u) % kFillHash;
    for (int probe = 0; probe < kFillHash; ++probe) {   // at most kTile / 2 distinct keys in kTile slots
      const int k = atomicCAS(&hkey[s], -1, key);
      if (k == -1 || k == key) {
        if (flag) atomicOr(&hflag[s], 1);
        if constexpr (LABEL) {
          if (lo <= hi) {
            atomicMin(&hlo[s], lo);
            atomicMax(&hhi[s], hi);
          }
          if (crosses) atomicOr(&hshared[s], 1);
        }
        return;
      }
      s = s + 1 == kFillHash ? 0 : s + 1;
    }
  };
  // label form: the thread's four values stay in registers -- its z-neighbours are its own, its x-neighbours and one of its
  // y-neighbours are other lanes' of the wavefront (two rows of 32), the rest (tile faces) comes from memory
  int v[kTD];
  if constexpr (LABEL) {
#pragma unroll
    for (int z = 0; z < kTD; ++z) {
      const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
      v[z] = gz < g.d && gy < g.h && gx < g.w ? (int)src[vbase + ((size_t)gz * g.h + gy) * g.w + gx] : 1;
    }
  }
#pragma unroll
  for (int z = 0; z < kTD; ++z) {
    const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
    const bool inside = gz < g.d && gy < g.h && gx < g.w;
    const size_t gi = vbase + ((size_t)gz * g.h + gy) * g.w + gx;   // dereferenced only when inside
    int a = inside ? par[gi] : -1;
    const bool member = a >= 0;
    bool border = false;
    if (member) {
      int p = par[a];
      for (long it = 0; p != a; ++it) {
        if (it > g.vv) { bad = true; break; }
        a = p;
        p = par[a];
      }
      par[gi] = a;
      border = gz == 0 || gy == 0 || gx == 0 || gz == g.d - 1 || gy == g.h - 1 || gx == g.w - 1;
    }
    int lo = INT_MAX, hi = INT_MIN;
    bool crosses = false;   // a zero neighbour in another tile: the component is not this tile's alone
    if constexpr (LABEL) {
      const int left = __shfl_up(v[z], 1, 64), right = __shfl_down(v[z], 1, 64);
      const int up = __shfl_up(v[z], kTW, 64), down = __shfl_down(v[z], kTW, 64);
      if (member) {
        auto see = [&](int nv) {
          if (nv != 0) {
            lo = min(lo, nv);
            hi = max(hi, nv);
          }
        };
        auto across = [&](size_t j, bool other_tile) {
          const int nv = (int)src[j];
          crosses |= other_tile && nv == 0;
          return nv;
        };
        if (gx > 0) see(x > 0 ? left : across(gi - 1, true));
        if (gx < g.w - 1) see(x < kTW - 1 ? right : across(gi + 1, true));
        if (gy > 0) see(lane >= kTW ? up : across(gi - g.w, y == 0));
        if (gy < g.h - 1) see(lane < kTW ? down : across(gi + g.w, y == kTH - 1));
        if (gz > 0) see(z > 0 ? v[z > 0 ? z - 1 : 0] : across(gi - hw, true));
        if (gz < g.d - 1) see(z < kTD - 1 ? v[z < kTD - 1 ? z + 1 : z] : across(gi + hw, true));
      }
    }
    // Lanes of one wavefront that bring something to the same root merge in registers first: a region's voxels all hit ONE
    // hash slot, and LDS atomics on one address serialise.  Up to four roots per wavefront and z (the leader's of the lanes
    // still waiting, a group of one goes straight in); whatever waits after that goes in lane by lane.
    bool has = member && (border || lo <= hi || crosses);
    unsigned long long todo = __ballot(has);
    for (int round = 0; round < 4 && todo; ++round) {   // wave-uniform
      const int leader = __ffsll(todo) - 1;
      const int key = __shfl(a, leader, 64);
      const bool mine = has && a == key;
      const unsigned long long grp = __ballot(mine);
      if (__popcll(grp) > 1) {
        const bool f = __ballot(mine && border) != 0, cr = __ballot(mine && crosses) != 0;
        int l = mine ? lo : INT_MAX, hh = mine ? hi : INT_MIN;
        if constexpr (LABEL) {
          for (int o = 32; o > 0; o >>= 1) {
            l = min(l, __shfl_xor(l, o, 64));
            hh = max(hh, __shfl_xor(hh, o, 64));
          }
        }
        if (lane == leader) insert(key, f, l, hh, cr);
      } else if (lane == leader) {
        insert(a, border, lo, hi, crosses);
      }
      has = has && !mine;
      todo &= ~grp;
    }
    if (has) insert(a, border, lo, hi, crosses);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kFillHash; i += kThreads) {
    const int k = hkey[i];
    if (k < 0) continue;
    int* wk = words + (size_t)W * k;
    if constexpr (LABEL) {
      // no voxel of the component has a zero neighbour across a tile face: all of it, its root included, lies in this tile
      // and nobody else sends anything for it -- plain stores.  (The many small holes of a prediction; an atomic on a word
      // of its own costs a trip to memory each.)
      if (!hshared[i]) {
        wk[0] = hflag[i];
        wk[1] = hlo[i];
        wk[2] = hhi[i];
        continue;
      }
    }
    if (hflag[i] && !ld_agent(&wk[0])) atomicOr(&wk[0], 1);
    if constexpr (LABEL) {
      if (hlo[i] < ld_agent(&wk[1])) atomicMin(&wk[1], hlo[i]);
      if (hhi[i] > ld_agent(&wk[2])) atomicMax(&wk[2], hhi[i]);
    }
  }
  if (bad) atomicOr(&status[vol], kStatusBound);
}

// apply (a new launch: the words are final, and no neighbour is read any more, so dst may be src): one streaming pass;
// blockIdx.y walks the volumes, so a workgroup's count of filled voxels belongs to one volume at a time -- registers, a
// wavefront reduction, LDS, then one atomic per workgroup and volume.
template <typename T, bool LABEL>
__global__ void __launch_bounds__(kThreads)
fill_apply_k(const T* src, int* dst, const int* __restrict__ par, const int* __restrict__ words, int* __restrict__ counts,
             long vv, int n, FillClasses cls) {
  __shared__ int wsum[kThreads / 64];
  const int tid = threadIdx.x;
  for (int vol = blockIdx.y; vol < n; vol += gridDim.y) {
    const size_t vbase = (size_t)vol * vv;
    int cnt = 0;
    for (long r = (long)blockIdx.x * kThreads + tid; r < vv; r += (long)gridDim.x * kThreads) {
      const size_t i = vbase + r;
      const T s = src[i];
      int out;
      if (s != (T)0) {
        out = LABEL ? (int)s : 1;
      } else {
        const int root = par ? par[i] : 0;
        bool fill;
        int c = 1;
        if constexpr (LABEL) {
          const int* wk = words + 3 * (size_t)root;
          fill = wk[0] == 0;
          if (fill) {
            c = wk[1];
            fill = c == wk[2];
          }
          if (fill && cls.n > 0) {
            bool in = false;
            for (int j = 0; j < cls.n; ++j) in |= cls.v[j] == c;
            fill = in;
          }
        } else {
          fill = words && words[root] == 0;   // words == nullptr (uniform): MSK_FILL_NONE, nothing is filled
        }
        out = fill ? c : 0;
        cnt += fill;
      }
      dst[i] = out;
    }
    if (counts) {   // uniform
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
      if (tid % 64 == 0) wsum[tid / 64] = cnt;
      __syncthreads();
      if (tid == 0) {
        int total = 0;
        for (int w = 0; w < kThreads / 64; ++w) total += wsum[w];
        if (total) atomicAdd(&counts[vol], total);
      }
      __syncthreads();
    }
  }
}

template <typename T, bool LABEL>
int run_fill(msk_ctx* ctx, const T* src, int32_t* dst, int n, int d, int h, int w, const FillClasses& cls, bool search,
             int32_t* status, int32_t* counts) {
  constexpr int W = LABEL ? 3 : 1;
  Geo g;
  g.d = d;
  g.h = h;
  g.w = w;
  g.tz = (d + kTD - 1) / kTD;
  g.ty = (h + kTH - 1) / kTH;
  g.tx = (w + kTW - 1) / kTW;
  g.vv = (long)d * h * w;
  const long T_ = (long)n * g.vv;
  int* par = nullptr;
  int* words = nullptr;
  if (search) {
    par = (int*)msk_workspace(ctx, (size_t)(1 + W) * T_ * sizeof(int));   // dst may be src: the links live in scratch
    if (!par) return -1;
    words = par + T_;
  }
  const long ntiles = (long)n * g.tz * g.ty * g.tx;
  hipStream_t st = ctx->stream;
  {
    msk_launch_scope ls(ctx, "fill_init");
    hipLaunchKernelGGL(ccl_init_k, dim3(std::max(1, std::min(64, (n + kThreads - 1) / kThreads))), dim3(kThreads), 0, st,
                       (int*)nullptr, status, counts, n);
    MSK_LAUNCH_CHECK(ctx);
  }
  if (search) {
    msk_launch_scope ls(ctx, "fill_local");
    hipLaunchKernelGGL((ccl_local_k<T, W>), dim3((unsigned)ntiles), dim3(kThreads), 0, st, src, par, words, (int*)nullptr,
                       status, g);
    MSK_LAUNCH_CHECK(ctx);
  }
  if (search) {
    msk_launch_scope ls(ctx, "fill_merge");
    hipLaunchKernelGGL(ccl_merge_k, dim3(msk_ew_blocks(T_, ctx->num_cu)), dim3(kThreads), 0, st, par, status, g, T_);
    MSK_LAUNCH_CHECK(ctx);
  }
  if (search) {
    msk_launch_scope ls(ctx, "fill_gather");
    hipLaunchKernelGGL((fill_gather_k<T, LABEL>), dim3((unsigned)ntiles), dim3(kThreads), 0, st, src, par, words, status, g);
    MSK_LAUNCH_CHECK(ctx);
  }
  {
    msk_launch_scope ls(ctx, "fill_apply");
    const unsigned bx = (unsigned)std::max(1, msk_ew_blocks(g.vv, ctx->num_cu) / std::min(n, 8));
    hipLaunchKernelGGL((fill_apply_k<T, LABEL>), dim3(bx, (unsigned)std::min(n, 65535)), dim3(kThreads), 0, st, src, dst,
                       (const int*)par, (const int*)words, counts, g.vv, n, cls);
    MSK_LAUNCH_CHECK(ctx);
  }
  return 0;
}

}  // namespace

extern "C" {

int msk_connected_components3d(msk_ctx* ctx, const void* src, int32_t* dst, int n, int d, int h, int w, int dtype,
                               int minimum_volume, int k, int32_t* status, int32_t* counts) {
  MSK_REQUIRE(ctx, dtype == 0 || dtype == 1, "dtype must be 0 (float32) or 1 (int32)");
  MSK_REQUIRE(ctx, n > 0 && d > 0 && h > 0 && w > 0, "empty volume");
  MSK_REQUIRE(ctx, (long)n * d * h * w <= (long)INT_MAX / 2, "n*d*h*w must stay below 2^30 (int32 voxel indices)");
  MSK_REQUIRE(ctx, src && dst && status, "src, dst and status are required");
  MSK_REQUIRE(ctx, src != (const void*)dst, "connected components are out of place");
  if (dtype == 0) return run_ccl(ctx, (const float*)src, dst, n, d, h, w, minimum_volume, k, status, counts);
  return run_ccl(ctx, (const int32_t*)src, dst, n, d, h, w, minimum_volume, k, status, counts);
}

int msk_fill_holes3d(msk_ctx* ctx, const void* src, int32_t* dst, int n, int d, int h, int w, int dtype, int mode,
                     const int32_t* classes, int nclasses, int32_t* status, int32_t* counts) {
  MSK_REQUIRE(ctx, dtype == 0 || dtype == 1, "dtype must be 0 (float32) or 1 (int32)");
  MSK_REQUIRE(ctx, mode == MSK_FILL_MASK || mode == MSK_FILL_LABEL || mode == MSK_FILL_NONE,
              "mode must be MSK_FILL_MASK, MSK_FILL_LABEL or MSK_FILL_NONE");
  MSK_REQUIRE(ctx, dtype == 1 || mode != MSK_FILL_LABEL, "a float32 volume has no label form");
  MSK_REQUIRE(ctx, n > 0 && d > 0 && h > 0 && w > 0, "empty volume");
  MSK_REQUIRE(ctx, (long)n * d * h * w <= (long)INT_MAX / 2, "n*d*h*w must stay below 2^30 (int32 voxel indices)");
  MSK_REQUIRE(ctx, src && dst && status, "src, dst and status are required");
  MSK_REQUIRE(ctx, nclasses >= 0 && nclasses <= kFillMaxClasses, "at most 64 classes");
  MSK_REQUIRE(ctx, nclasses == 0 || classes, "classes is null");
  MSK_REQUIRE(ctx, nclasses == 0 || mode == MSK_FILL_LABEL, "only MSK_FILL_LABEL takes classes");
  const size_t bytes = (size_t)n * d * h * w * 4;
  const char *sb = (const char*)src, *db = (const char*)dst;
  MSK_REQUIRE(ctx, (sb == db && dtype == 1) || sb + bytes <= db || db + bytes <= sb,
              "dst may be src itself (int32 only) and must not overlap it otherwise");
  FillClasses cls;
  cls.n = nclasses;
  for (int i = 0; i < kFillMaxClasses; ++i) cls.v[i] = i < nclasses ? classes[i] : 0;
  const bool search = mode != MSK_FILL_NONE;
  if (dtype == 0) return run_fill<float, false>(ctx, (const float*)src, dst, n, d, h, w, cls, search, status, counts);
  if (mode != MSK_FILL_LABEL)
    return run_fill<int32_t, false>(ctx, (const int32_t*)src, dst, n, d, h, w, cls, search, status, counts);
  return run_fill<int32_t, true>(ctx, (const int32_t*)src, dst, n, d, h, w, cls, true, status, counts);
}

}  // extern "C"
