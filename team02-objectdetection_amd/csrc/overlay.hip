// Post-processing of the reference's overlay_predictions (inference.py:72-146) on the GPU:
//
//   road = (cls == 1) -> 5x5 morphological close -> 8-connected components -> largest ->
//   cleaned = cls with the largest road component painted 1 -> class colours -> car blobs
//   (components of cleaned == 2) with bounding boxes -> 0.6 / 0.4 blend -> box outlines.
//
// Everything is stream-ordered on the caller's stream, with no host round trip, so the whole
// stage is one chain of launches that a graph capture records as it is.  Every result is
// independent of scheduling: labels are the smallest linear index of the component (links by
// atomicMin), areas are integer atomicAdd, boxes atomicMin / atomicMax, the largest component an
// atomicMax on (area << 32) | ~root, the box list an ordered compaction (no atomic append).
//
// cv2 is not installed in this image: the close (constant border: pixels outside the image never
// decide), the blend (cv2.addWeighted's 8-bit path as published: two float32 products, a float32
// sum, round half to even) and the labelling are restated; tests pin kernel == restatement.
#include "common.h"

#include <limits.h>

namespace {

typedef unsigned long long u64;

constexpr int kCcTH = 16, kCcTW = 64;  // labelling tile (seg_cc_tile_h / seg_cc_tile_w)

// ---------------------------------------------------------------- 5x5 close, bit-packed
// A block closes kClTR rows x (64 * kClKW) columns.  Row words: [0] the 64 pixels left of the tile, [1..KW] the
// tile, [KW + 1] the 64 pixels right of it; rows: 4 above .. 4 below (2 for the dilation + 2 for the erosion).
constexpr int kClTR = 16, kClKW = 4, kClRows = kClTR + 8, kClWords = kClKW + 2;

__device__ __forceinline__ u64 row5_or(u64 l, u64 w, u64 r) {
  return w | (w << 1) | (w << 2) | (l >> 63) | (l >> 62) | (w >> 1) | (w >> 2) | (r << 63) | (r << 62);
}
__device__ __forceinline__ u64 row5_and(u64 l, u64 w, u64 r) {
  return w & ((w << 1) | (l >> 63)) & ((w << 2) | (l >> 62)) & ((w >> 1) | (r << 63)) & ((w >> 2) | (r << 62));
}

__global__ __launch_bounds__(256) void close5_kernel(const uint8_t* __restrict__ src, int Hf, int Wf, int cls,
                                                     uint8_t* __restrict__ out) {
  __shared__ u64 a[kClRows][kClWords], b[kClRows][kClWords];
  const int x0 = blockIdx.x * (64 * kClKW), y0 = blockIdx.y * kClTR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t = threadIdx.x;
  // raw road bits, one ballot per word; outside the image: 0 (never decides the dilation)
  for (int i = wave; i < kClRows * kClWords; i += 4) {
    const int r = i / kClWords, k = i - r * kClWords;
    const int y = y0 - 4 + r, x = x0 + (k - 1) * 64 + lane;
    const bool on = y >= 0 && y < Hf && x >= 0 && x < Wf && src[(long)y * Wf + x] == cls;
    const u64 m = __ballot(on);
    if (lane == 0) a[r][k] = m;
  }
  __syncthreads();
  // horizontal OR (the outer 2 bits of the two neighbour words lack a carry; they are never used)
  if (t < kClRows * kClWords) {
    const int r = t / kClWords, k = t - r * kClWords;
    b[r][k] = row5_or(k > 0 ? a[r][k - 1] : 0, a[r][k], k < kClWords - 1 ? a[r][k + 1] : 0);
  }
  __syncthreads();
  // vertical OR = the dilation; then outside the image: 1 (never decides the erosion)
  if (t < kClRows * kClWords) {
    const int r = t / kClWords, k = t - r * kClWords;
    u64 v = 0;
    if (r >= 2 && r < kClRows - 2) {
      const int y = y0 - 4 + r;
      v = b[r - 2][k] | b[r - 1][k] | b[r][k] | b[r + 1][k] | b[r + 2][k];
      const int xw = x0 + (k - 1) * 64;  // column of bit 0, a multiple of 64: the word starts inside or lies outside
      u64 outside = 0;
      if (y < 0 || y >= Hf || xw < 0 || xw >= Wf) outside = ~0ull;
      else if (xw + 63 >= Wf) outside = ~0ull << (Wf - xw);
      v |= outside;
    }
    a[r][k] = v;
  }
  __syncthreads();
  if (t < kClRows * kClWords) {
    const int r = t / kClWords, k = t - r * kClWords;
    b[r][k] = (k >= 1 && k <= kClKW) ? row5_and(a[r][k - 1], a[r][k], a[r][k + 1]) : 0;
  }
  __syncthreads();
  if (t < kClTR * kClKW) {
    const int r = 4 + t / kClKW, k = 1 + t % kClKW;
    a[r][k] = b[r - 2][k] & b[r - 1][k] & b[r][k] & b[r + 1][k] & b[r + 2][k];
  }
  __syncthreads();
  for (int i = t; i < kClTR * kClKW * 64; i += 256) {
    const int r = i / (kClKW * 64), xl = i - r * (kClKW * 64);
    const int y = y0 + r, x = x0 + xl;
    if (y < Hf && x < Wf) out[(long)y * Wf + x] = (uint8_t)((a[4 + r][1 + (xl >> 6)] >> (xl & 63)) & 1);
  }
}

// ---------------------------------------------------------------- labelling: tiled union-find
// The unions of pixel p, decided on the whole image: with its N neighbour if set (W, NW and NE then reach N
// through their own unions); otherwise with W, or NW if W is clear, and with NE.  The tile kernel makes the
// unions whose two ends lie in one tile, the border kernel the others.  Bits: 1 W, 2 NW, 4 N, 8 NE.
__device__ __forceinline__ int cc_links(bool n, bool w, bool nw, bool ne) {
  return n ? 4 : ((w ? 1 : (nw ? 2 : 0)) | (ne ? 8 : 0));
}

__device__ __forceinline__ bool cc_fg(uint8_t v, int match) { return match < 0 ? v != 0 : v == match; }

// Parents only ever decrease and always stay inside the component, so any value read is an ancestor.
__device__ __forceinline__ int cc_ld(const int* p) {
  return __hip_atomic_load(const_cast<int*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int cc_find(const int* par, int a) {
  for (int p = cc_ld(par + a); p != a; p = cc_ld(par + a)) a = p;
  return a;
}
// Link the larger root under the smaller.  If `a` stopped being a root meanwhile, the atomicMin still keeps the
// smaller parent and the displaced one (`old`) is united with b in the next round: no link is lost.
__device__ __forceinline__ void cc_unite(int* par, int a, int b) {
  for (;;) {
    a = cc_find(par, a);
    b = cc_find(par, b);
    if (a == b) return;
    if (a < b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(par + a, b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(256) void cc_tile_kernel(const uint8_t* __restrict__ src, int Hf, int Wf, int match,
                                                      int* __restrict__ lab) {
  __shared__ int par[kCcTH * kCcTW];
  __shared__ uint8_t fg[kCcTH + 1][kCcTW + 2];  // rows y0-1 .., columns x0-1 .. x0+TW
  const int x0 = blockIdx.x * kCcTW, y0 = blockIdx.y * kCcTH;
  for (int i = threadIdx.x; i < (kCcTH + 1) * (kCcTW + 2); i += 256) {
    const int r = i / (kCcTW + 2), c = i - r * (kCcTW + 2);
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    fg[r][c] = y >= 0 && y < Hf && x >= 0 && x < Wf && cc_fg(src[(long)y * Wf + x], match);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kCcTH * kCcTW; i += 256) {
    const int ly = i / kCcTW, lx = i - ly * kCcTW;
    par[i] = fg[ly + 1][lx + 1] ? i : -1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kCcTH * kCcTW; i += 256) {
    const int ly = i / kCcTW, lx = i - ly * kCcTW;
    if (!fg[ly + 1][lx + 1]) continue;
    const int sel = cc_links(fg[ly][lx + 1], fg[ly + 1][lx], fg[ly][lx], fg[ly][lx + 2]);
    if ((sel & 4) && ly > 0) cc_unite(par, i, i - kCcTW);
    if ((sel & 1) && lx > 0) cc_unite(par, i, i - 1);
    if ((sel & 2) && ly > 0 && lx > 0) cc_unite(par, i, i - kCcTW - 1);
    if ((sel & 8) && ly > 0 && lx < kCcTW - 1) cc_unite(par, i, i - kCcTW + 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kCcTH * kCcTW; i += 256) {
    const int ly = i / kCcTW, lx = i - ly * kCcTW;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= Hf || x >= Wf) continue;
    int g = -1;
    if (par[i] >= 0) {
      const int r = cc_find(par, i);
      g = (y0 + r / kCcTW) * Wf + x0 + r % kCcTW;
    }
    lab[(long)y * Wf + x] = g;
  }
}

__global__ __launch_bounds__(256) void cc_border_kernel(int* __restrict__ lab, int Hf, int Wf) {
  const int total = Hf * Wf;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const int y = p / Wf, x = p - y * Wf;
  const int ly = y % kCcTH, lx = x % kCcTW;
  if (ly != 0 && lx != 0 && lx != kCcTW - 1) return;
  if (cc_ld(lab + p) < 0) return;
  const bool n = y > 0 && cc_ld(lab + p - Wf) >= 0;
  const bool w = x > 0 && cc_ld(lab + p - 1) >= 0;
  const bool nw = y > 0 && x > 0 && cc_ld(lab + p - Wf - 1) >= 0;
  const bool ne = y > 0 && x < Wf - 1 && cc_ld(lab + p - Wf + 1) >= 0;
  const int sel = cc_links(n, w, nw, ne);
  if ((sel & 4) && ly == 0) cc_unite(lab, p, p - Wf);
  if ((sel & 1) && lx == 0) cc_unite(lab, p, p - 1);
  if ((sel & 2) && (ly == 0 || lx == 0)) cc_unite(lab, p, p - Wf - 1);
  if ((sel & 8) && (ly == 0 || lx == kCcTW - 1)) cc_unite(lab, p, p - Wf + 1);
}

// Every set pixel takes its root.  With `area` the root's statistics are reset here (the per-frame clearing of
// the stage: only root entries are ever read); with `key` the largest-component word.
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* __restrict__ lab, int total, int* __restrict__ area,
                                                         int* __restrict__ box, u64* __restrict__ key) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p == 0 && key) *key = 0;
  if (p >= total) return;
  if (cc_ld(lab + p) < 0) return;
  const int r = cc_find(lab, p);
  if (r != p) {
    __hip_atomic_store(lab + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (area) area[p] = 0;
  if (box) {
    box[4L * p + 0] = INT_MAX;
    box[4L * p + 1] = INT_MAX;
    box[4L * p + 2] = -1;
    box[4L * p + 3] = -1;
  }
}

// The same reset for labels that are already flat (the op-level entries).
__global__ __launch_bounds__(256) void cc_reset_kernel(const int* __restrict__ lab, int total, int* __restrict__ area,
                                                       int* __restrict__ box, u64* __restrict__ key) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p == 0 && key) *key = 0;
  if (p >= total || lab[p] != p) return;
  area[p] = 0;
  if (box) {
    box[4L * p + 0] = INT_MAX;
    box[4L * p + 1] = INT_MAX;
    box[4L * p + 2] = -1;
    box[4L * p + 3] = -1;
  }
}

// ---------------------------------------------------------------- areas and boxes
struct CcRun {
  int root, cnt, x0, y0, x1, y1;
};

template <bool BOX>
__device__ __forceinline__ void cc_flush(const CcRun& r, int* area, int* box) {
  atomicAdd(area + r.root, r.cnt);
  if (BOX) {
    atomicMin(box + 4L * r.root + 0, r.x0);
    atomicMin(box + 4L * r.root + 1, r.y0);
    atomicMax(box + 4L * r.root + 2, r.x1);
    atomicMax(box + 4L * r.root + 3, r.y1);
  }
}

// A thread walks kStatRun consecutive pixels and keeps the run of its current root in registers, so one large
// component costs a thread one flush; the final flushes of a wave that share a root are combined first (one set
// of atomics per wave and root: all pixels of a frame-sized road would otherwise queue on one address).
constexpr int kStatRun = 16;
template <bool BOX>
__global__ __launch_bounds__(256) void cc_stats_kernel(const int* __restrict__ lab, int Wf, int total,
                                                       int* __restrict__ area, int* __restrict__ box) {
  const long base = ((long)blockIdx.x * 256 + threadIdx.x) * kStatRun;
  CcRun run = {-1, 0, INT_MAX, INT_MAX, -1, -1};
  if (base < total) {
    int y = (int)(base / Wf), x = (int)(base - (long)y * Wf);
    const int n = (int)std::min<long>(kStatRun, total - base);
    for (int j = 0; j < n; ++j) {
      const int r = lab[base + j];
      if (r >= 0) {
        if (r != run.root) {
          if (run.root >= 0) cc_flush<BOX>(run, area, box);
          run = {r, 0, INT_MAX, INT_MAX, -1, -1};
        }
        ++run.cnt;
        run.x0 = min(run.x0, x);
        run.y0 = min(run.y0, y);
        run.x1 = max(run.x1, x);
        run.y1 = max(run.y1, y);
      }
      if (++x == Wf) {
        x = 0;
        ++y;
      }
    }
  }
  const int lane = threadIdx.x & 63;
  for (;;) {  // wave-uniform: every lane of the wave is here
    const u64 live = __ballot(run.root >= 0);
    if (!live) break;
    const int leader = __ffsll((long long)live) - 1;
    const int root = __shfl(run.root, leader, 64);
    const bool mine = run.root == root;
    CcRun s = mine ? run : CcRun{root, 0, INT_MAX, INT_MAX, -1, -1};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s.cnt += __shfl_xor(s.cnt, o, 64);
      if (BOX) {
        s.x0 = min(s.x0, __shfl_xor(s.x0, o, 64));
        s.y0 = min(s.y0, __shfl_xor(s.y0, o, 64));
        s.x1 = max(s.x1, __shfl_xor(s.x1, o, 64));
        s.y1 = max(s.y1, __shfl_xor(s.y1, o, 64));
      }
    }
    if (lane == leader) cc_flush<BOX>(s, area, box);
    if (mine) run.root = -1;
  }
}

// key = max over roots of (area << 32) | (0xFFFFFFFF - root): the largest area, then the smallest root.
__global__ __launch_bounds__(256) void cc_largest_kernel(const int* __restrict__ lab, int total,
                                                         const int* __restrict__ area, u64* __restrict__ key) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  u64 k = 0;
  if (p < total && lab[p] == p) k = ((u64)(unsigned)area[p] << 32) | (u64)(0xFFFFFFFFu - (unsigned)p);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 other = ((u64)(unsigned)__shfl_xor((int)(k >> 32), o, 64) << 32) |
                      (u64)(unsigned)__shfl_xor((int)(k & 0xFFFFFFFFu), o, 64);
    k = other > k ? other : k;
  }
  if ((threadIdx.x & 63) == 0 && k) atomicMax(key, k);
}

__global__ void cc_largest_out_kernel(const u64* __restrict__ key, int* __restrict__ out) {
  const u64 k = *key;
  out[0] = k ? (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFu)) : -1;
  out[1] = (int)(k >> 32);
}

// cleaned = cls, the largest road component painted 1 (inference.py:105-106)
__global__ __launch_bounds__(256) void fill_kernel(const uint8_t* __restrict__ cls, const int* __restrict__ lab,
                                                   const u64* __restrict__ key, int total,
                                                   uint8_t* __restrict__ cleaned) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const u64 k = *key;
  const int root = k ? (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFu)) : -2;
  cleaned[p] = lab[p] == root ? (uint8_t)1 : cls[p];
}

// ---------------------------------------------------------------- box list: ordered compaction
__device__ __forceinline__ bool box_passes(const int* lab, const int* area, int p, int total, int min_area) {
  return p < total && lab[p] == p && area[p] > min_area;
}

__global__ __launch_bounds__(256) void box_count_kernel(const int* __restrict__ lab, const int* __restrict__ area,
                                                        int total, int min_area, int* __restrict__ blk) {
  __shared__ int wsum[4];
  const int p = blockIdx.x * 256 + threadIdx.x;
  const u64 m = __ballot(box_passes(lab, area, p, total, min_area));
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One block: blk[] -> its exclusive prefix sums; count = {stored, passed}.
__global__ __launch_bounds__(1024) void box_scan_kernel(int* __restrict__ blk, int nblk, int max_boxes,
                                                        int* __restrict__ count) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int per = (nblk + 1023) / 1024;
  const int lo = min(t * per, nblk), hi = min(lo + per, nblk);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += blk[i];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;  // exclusive
  for (int i = lo; i < hi; ++i) {
    const int v = blk[i];
    blk[i] = run;
    run += v;
  }
  if (t == 1023) {
    count[0] = min(part[t], max_boxes);
    count[1] = part[t];
  }
}

__global__ __launch_bounds__(256) void box_write_kernel(const int* __restrict__ lab, const int* __restrict__ area,
                                                        const int* __restrict__ box, int total, int min_area,
                                                        const int* __restrict__ blk, int max_boxes,
                                                        int* __restrict__ boxes) {
  __shared__ int wsum[4];
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool on = box_passes(lab, area, p, total, min_area);
  const u64 m = __ballot(on);
  if (lane == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  if (!on) return;
  int rank = blk[blockIdx.x] + __popcll(m & ((1ull << lane) - 1));
  for (int w = 0; w < wave; ++w) rank += wsum[w];
  if (rank >= max_boxes) return;
  const int x0 = box[4L * p], y0 = box[4L * p + 1];
  int* o = boxes + 5L * rank;
  o[0] = x0;
  o[1] = y0;
  o[2] = box[4L * p + 2] - x0 + 1;
  o[3] = box[4L * p + 3] - y0 + 1;
  o[4] = area[p];
}

// ---------------------------------------------------------------- colour + blend, outlines
// cv2.addWeighted(image, 0.6, overlay, 0.4, 0) on uint8: rint(float(a) * 0.6f + float(b) * 0.4f), each product
// and the sum rounded to float32 (no fused multiply-add), half to even.  At most 255, never negative.
__device__ __forceinline__ unsigned blend8(unsigned a, unsigned b) {
  return (unsigned)(int)rintf(__fadd_rn(__fmul_rn((float)a, 0.6f), __fmul_rn((float)b, 0.4f)));
}

// table: [ncolors][4] bytes = the class's colour in the frame's channel order and a "listed" flag; a class that
// is not listed, or >= ncolors, keeps the frame's pixel (overlay = image).
__global__ __launch_bounds__(256) void blend_kernel(const uint8_t* __restrict__ frame,
                                                    const uint8_t* __restrict__ cleaned, int total,
                                                    const uint8_t* __restrict__ table, int ncolors,
                                                    uint8_t* __restrict__ result, int vec) {
  __shared__ unsigned tab[256];
  {
    const int c = threadIdx.x;
    unsigned v = 0;
    if (c < ncolors) v = table[4 * c] | (table[4 * c + 1] << 8) | (table[4 * c + 2] << 16) | (table[4 * c + 3] ? 1u << 24 : 0u);
    tab[c] = v;
  }
  __syncthreads();
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= total) return;
  if (vec && p0 + 4 <= total) {  // 4 pixels = 12 bytes = 3 aligned words in, 3 out
    const unsigned* f = reinterpret_cast<const unsigned*>(frame + 3 * p0);
    const unsigned cw = *reinterpret_cast<const unsigned*>(cleaned + p0);
    unsigned in[3] = {f[0], f[1], f[2]}, out[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned e = tab[(cw >> (8 * j)) & 255u];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int byte = 3 * j + c;
        const unsigned a = (in[byte >> 2] >> (8 * (byte & 3))) & 255u;
        const unsigned bcol = (e >> 24) ? (e >> (8 * c)) & 255u : a;
        out[byte >> 2] |= blend8(a, bcol) << (8 * (byte & 3));
      }
    }
    unsigned* o = reinterpret_cast<unsigned*>(result + 3 * p0);
    o[0] = out[0];
    o[1] = out[1];
    o[2] = out[2];
    return;
  }
  for (long p = p0; p < p0 + 4 && p < total; ++p) {
    const unsigned e = tab[cleaned[p]];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned a = frame[3 * p + c];
      result[3 * p + c] = (uint8_t)blend8(a, (e >> 24) ? (e >> (8 * c)) & 255u : a);
    }
  }
}

// One block per stored box: the pixels of [x, x+w] x [y, y+h] (clipped to the frame) outside the inner rectangle
// [x+2, x+w-2] x [y+2, y+h-2] = rows y, y+1, y+h-1, y+h and columns x, x+1, x+w-1, x+w of it, become
// blend(image, green).  The value depends on the frame alone, so overlapping outlines agree.
__global__ __launch_bounds__(256) void outline_kernel(const uint8_t* __restrict__ frame, int Hf, int Wf,
                                                      const int* __restrict__ boxes, const int* __restrict__ count,
                                                      int max_boxes, uint8_t* __restrict__ result) {
  const int b = blockIdx.x;
  if (b >= min(count[0], max_boxes)) return;
  const int x = boxes[5 * b], y = boxes[5 * b + 1], w = boxes[5 * b + 2], h = boxes[5 * b + 3];
  const int nrow = 4 * (w + 1), ncol = 4 * (h + 1);
  for (int i = threadIdx.x; i < nrow + ncol; i += 256) {
    int px, py;
    if (i < nrow) {
      const int k = i / (w + 1);
      px = x + i - k * (w + 1);
      py = k == 0 ? y : (k == 1 ? y + 1 : (k == 2 ? y + h - 1 : y + h));
    } else {
      const int j = i - nrow, k = j / (h + 1);
      py = y + j - k * (h + 1);
      px = k == 0 ? x : (k == 1 ? x + 1 : (k == 2 ? x + w - 1 : x + w));
    }
    if (px < 0 || px >= Wf || py < 0 || py >= Hf) continue;
    const long o = 3 * ((long)py * Wf + px);
    result[o + 0] = (uint8_t)blend8(frame[o + 0], 0);
    result[o + 1] = (uint8_t)blend8(frame[o + 1], 255);
    result[o + 2] = (uint8_t)blend8(frame[o + 2], 0);
  }
}

// ---------------------------------------------------------------- host side
inline long r16(long v) { return (v + 15) & ~15L; }

struct Workspace {  // byte offsets into the caller's buffer
  long key, closed, labels, area, box, blk, bytes;
};

bool dims_ok(int Hf, int Wf) { return Hf > 0 && Wf > 0 && (long)Hf * Wf < (1L << 31); }

Workspace layout(int Hf, int Wf) {
  const long hw = (long)Hf * Wf;
  Workspace w;
  w.key = 0;
  w.closed = 16;
  w.labels = w.closed + r16(hw);
  w.area = w.labels + r16(4 * hw);
  w.box = w.area + r16(4 * hw);
  w.blk = w.box + 16 * hw;
  w.bytes = w.blk + r16(4L * seg_cdiv(hw, 256));
  return w;
}

template <typename T>
T* at(void* work, long off) { return reinterpret_cast<T*>(static_cast<char*>(work) + off); }

int px_blocks(int total) { return seg_cdiv(total, 256); }

#define OV_CHECK()                                 \
  do {                                             \
    const hipError_t e_ = hipGetLastError();       \
    if (e_ != hipSuccess) return (int)e_;          \
  } while (0)

int launch_close(const uint8_t* mask, int Hf, int Wf, int cls, uint8_t* out, hipStream_t s) {
  hipLaunchKernelGGL(close5_kernel, dim3(seg_cdiv(Wf, 64 * kClKW), seg_cdiv(Hf, kClTR)), dim3(256), 0, s, mask, Hf,
                     Wf, cls, out);
  SEG_RET_LAST();
}

// 3 launches; area / box / key (each optional) are reset for the labels' roots by the last one.
int launch_label(const uint8_t* mask, int Hf, int Wf, int match, int* lab, int* area, int* box, u64* key,
                 hipStream_t s) {
  const int total = Hf * Wf;
  hipLaunchKernelGGL(cc_tile_kernel, dim3(seg_cdiv(Wf, kCcTW), seg_cdiv(Hf, kCcTH)), dim3(256), 0, s, mask, Hf, Wf,
                     match, lab);
  OV_CHECK();
  hipLaunchKernelGGL(cc_border_kernel, dim3(px_blocks(total)), dim3(256), 0, s, lab, Hf, Wf);
  OV_CHECK();
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(px_blocks(total)), dim3(256), 0, s, lab, total, area, box, key);
  SEG_RET_LAST();
}

int launch_stats(const int* lab, int Hf, int Wf, int* area, int* box, hipStream_t s) {
  const int total = Hf * Wf;
  const int blocks = seg_cdiv(total, 256L * kStatRun);
  if (box)
    hipLaunchKernelGGL(cc_stats_kernel<true>, dim3(blocks), dim3(256), 0, s, lab, Wf, total, area, box);
  else
    hipLaunchKernelGGL(cc_stats_kernel<false>, dim3(blocks), dim3(256), 0, s, lab, Wf, total, area, box);
  SEG_RET_LAST();
}

int launch_boxes(const int* lab, int total, const int* area, const int* box, int min_area, int max_boxes, int* blk,
                 int* boxes, int* count, hipStream_t s) {
  const int nblk = px_blocks(total);
  hipLaunchKernelGGL(box_count_kernel, dim3(nblk), dim3(256), 0, s, lab, area, total, min_area, blk);
  OV_CHECK();
  hipLaunchKernelGGL(box_scan_kernel, dim3(1), dim3(1024), 0, s, blk, nblk, max_boxes, count);
  OV_CHECK();
  hipLaunchKernelGGL(box_write_kernel, dim3(nblk), dim3(256), 0, s, lab, area, box, total, min_area, blk, max_boxes,
                     boxes);
  SEG_RET_LAST();
}

int launch_blend(const uint8_t* frame, const uint8_t* cleaned, int total, const uint8_t* table, int ncolors,
                 uint8_t* result, hipStream_t s) {
  const int vec = (((uintptr_t)frame | (uintptr_t)cleaned | (uintptr_t)result) & 3) == 0;
  hipLaunchKernelGGL(blend_kernel, dim3(seg_cdiv(total, 1024)), dim3(256), 0, s, frame, cleaned, total, table,
                     ncolors, result, vec);
  SEG_RET_LAST();
}

int launch_outline(const uint8_t* frame, int Hf, int Wf, const int* boxes, const int* count, int max_boxes,
                   uint8_t* result, hipStream_t s) {
  hipLaunchKernelGGL(outline_kernel, dim3(max_boxes), dim3(256), 0, s, frame, Hf, Wf, boxes, count, max_boxes,
                     result);
  SEG_RET_LAST();
}

constexpr int kMaxBoxes = 65535;

}  // namespace

SEG_API int seg_cc_tile_h(void) { return kCcTH; }
SEG_API int seg_cc_tile_w(void) { return kCcTW; }

// Bytes of the caller-owned workspace of seg_overlay_frame, seg_cc_largest and seg_cc_boxes; 0 for invalid sizes.
SEG_API long seg_overlay_workspace_bytes(int Hf, int Wf, int max_boxes) {
  if (!dims_ok(Hf, Wf) || max_boxes <= 0 || max_boxes > kMaxBoxes) return 0;
  return layout(Hf, Wf).bytes;
}

SEG_API int seg_morph_close5(const unsigned char* mask, int Hf, int Wf, int class_id, unsigned char* out,
                             hipStream_t stream) {
  if (!dims_ok(Hf, Wf) || !mask || !out || class_id < 0 || class_id > 255) return (int)hipErrorInvalidValue;
  return launch_close(mask, Hf, Wf, class_id, out, stream);
}

SEG_API int seg_cc_label8(const unsigned char* mask, int Hf, int Wf, int* labels, hipStream_t stream) {
  if (!dims_ok(Hf, Wf) || !mask || !labels) return (int)hipErrorInvalidValue;
  return launch_label(mask, Hf, Wf, -1, labels, nullptr, nullptr, nullptr, stream);
}

SEG_API int seg_cc_largest(const int* labels, int Hf, int Wf, int* out, void* work, long work_bytes,
                           hipStream_t stream) {
  if (!dims_ok(Hf, Wf) || !labels || !out || !work || ((uintptr_t)work & 15) || work_bytes < layout(Hf, Wf).bytes)
    return (int)hipErrorInvalidValue;
  const Workspace w = layout(Hf, Wf);
  const int total = Hf * Wf;
  int* area = at<int>(work, w.area);
  u64* key = at<u64>(work, w.key);
  hipLaunchKernelGGL(cc_reset_kernel, dim3(px_blocks(total)), dim3(256), 0, stream, labels, total, area,
                     (int*)nullptr, key);
  OV_CHECK();
  int rc = launch_stats(labels, Hf, Wf, area, nullptr, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(cc_largest_kernel, dim3(px_blocks(total)), dim3(256), 0, stream, labels, total, area, key);
  OV_CHECK();
  hipLaunchKernelGGL(cc_largest_out_kernel, dim3(1), dim3(1), 0, stream, key, out);
  SEG_RET_LAST();
}

SEG_API int seg_cc_boxes(const int* labels, int Hf, int Wf, int min_area, int max_boxes, int* boxes, int* count,
                         void* work, long work_bytes, hipStream_t stream) {
  if (!dims_ok(Hf, Wf) || max_boxes <= 0 || max_boxes > kMaxBoxes || !labels || !boxes || !count || !work ||
      work_bytes < layout(Hf, Wf).bytes)
    return (int)hipErrorInvalidValue;
  const Workspace w = layout(Hf, Wf);
  const int total = Hf * Wf;
  int* area = at<int>(work, w.area);
  int* box = at<int>(work, w.box);
  hipLaunchKernelGGL(cc_reset_kernel, dim3(px_blocks(total)), dim3(256), 0, stream, labels, total, area, box,
                     (u64*)nullptr);
  OV_CHECK();
  int rc = launch_stats(labels, Hf, Wf, area, box, stream);
  if (rc) return rc;
  return launch_boxes(labels, total, area, box, min_area, max_boxes, at<int>(work, w.blk), boxes, count, stream);
}

SEG_API int seg_overlay_blend(const unsigned char* frame, const unsigned char* cleaned, int Hf, int Wf,
                              const unsigned char* table, int ncolors, unsigned char* result, hipStream_t stream) {
  if (!dims_ok(Hf, Wf) || !frame || !cleaned || !result || ncolors < 0 || ncolors > 256 || (ncolors && !table))
    return (int)hipErrorInvalidValue;
  return launch_blend(frame, cleaned, Hf * Wf, table, ncolors, result, stream);
}

SEG_API int seg_overlay_outline(const unsigned char* frame, int Hf, int Wf, const int* boxes, const int* count,
                                int max_boxes, unsigned char* result, hipStream_t stream) {
  if (!dims_ok(Hf, Wf) || max_boxes <= 0 || max_boxes > kMaxBoxes || !frame || !boxes || !count || !result)
    return (int)hipErrorInvalidValue;
  return launch_outline(frame, Hf, Wf, boxes, count, max_boxes, result, stream);
}

// The whole stage, 16 launches (15 without outlines) in one chain on `stream`:
//   close 1, road labels 3, road areas 1, largest 1, fill 1, car labels 3, car areas + boxes 1, box list 3,
//   colour + blend 1, outlines 1.
SEG_API int seg_overlay_frame(const unsigned char* frame, const unsigned char* cls, int Hf, int Wf,
                              const unsigned char* table, int ncolors, int min_area, int max_boxes, int draw_boxes,
                              unsigned char* cleaned, unsigned char* result, int* boxes, int* count, void* work,
                              long work_bytes, hipStream_t stream) {
  if (!dims_ok(Hf, Wf) || max_boxes <= 0 || max_boxes > kMaxBoxes || !frame || !cls || !cleaned || !result ||
      !boxes || !count || !work || ncolors < 0 || ncolors > 256 || (ncolors && !table) ||
      ((uintptr_t)work & 15) || work_bytes < layout(Hf, Wf).bytes)
    return (int)hipErrorInvalidValue;
  const Workspace w = layout(Hf, Wf);
  const int total = Hf * Wf;
  uint8_t* closed = at<uint8_t>(work, w.closed);
  int* lab = at<int>(work, w.labels);
  int* area = at<int>(work, w.area);
  int* box = at<int>(work, w.box);
  u64* key = at<u64>(work, w.key);
  int rc;
  if ((rc = launch_close(cls, Hf, Wf, 1, closed, stream))) return rc;
  if ((rc = launch_label(closed, Hf, Wf, -1, lab, area, nullptr, key, stream))) return rc;
  if ((rc = launch_stats(lab, Hf, Wf, area, nullptr, stream))) return rc;
  hipLaunchKernelGGL(cc_largest_kernel, dim3(px_blocks(total)), dim3(256), 0, stream, lab, total, area, key);
  OV_CHECK();
  hipLaunchKernelGGL(fill_kernel, dim3(px_blocks(total)), dim3(256), 0, stream, cls, lab, key, total, cleaned);
  OV_CHECK();
  if ((rc = launch_label(cleaned, Hf, Wf, 2, lab, area, box, nullptr, stream))) return rc;
  if ((rc = launch_stats(lab, Hf, Wf, area, box, stream))) return rc;
  if ((rc = launch_boxes(lab, total, area, box, min_area, max_boxes, at<int>(work, w.blk), boxes, count, stream)))
    return rc;
  if ((rc = launch_blend(frame, cleaned, total, table, ncolors, result, stream))) return rc;
  if (draw_boxes) return launch_outline(frame, Hf, Wf, boxes, count, max_boxes, result, stream);
  return 0;
}
