// turns.hip -- the four symmetries of a rectangle that swap width and height, made on the device from ONE read of an
// uploaded image: the quarter turns (8 = clockwise, QTransform().rotate(90); 16 = counter-clockwise) and the transposes
// (32 = main diagonal, 64 = anti-diagonal).  Together with mirror.hip's reflections (1, 2, 4) they are the eight views a
// needle can be searched in; the DCT hash sees none of them in the other ("DCT hashes do not support rotation",
// src/dctfeaturesindex.h:34), so each view is processed as an image of its own.  k_turn_views writes the grey planes of
// the requested views, h columns by w rows, and with the colour leg the turned colour images.
//
// A workgroup of 256 owns a 64 x 64 tile of the source.  Load: a thread owns 16 consecutive pixels of one tile row (16 * CH
// bytes in CH 16-byte loads where the row is 16-byte aligned, byte by byte elsewhere and at the ragged right edge, as
// mirror.hip does), makes their 16 grey bytes and writes them to the LDS tile with one ds_write_b128.  Store: a thread
// owns one source column and 16 consecutive source rows = 16 consecutive pixels of one destination row; it gathers them
// from LDS byte by byte into four dwords, and every view is a store of those dwords: reversed in registers (v_perm_b32)
// for 8 and 64, whose destination rows run against the source rows, to row w-1-x instead of x for 16 and 64.  One
// 16-byte store where the destination is aligned (rows are h bytes long, so that depends on h % 16 and the row); where
// it is not, the widest stores the address allows (put16), byte stores for ragged chunks.  Four adjacent lanes write 64
// consecutive bytes of one destination row; the other half of that 128-byte line belongs to the tile below, so the grid
// is one-dimensional and numbered so that the workgroups of one XCD walk down the columns of tiles (see the kernel).
// Measured in NOTES.md: with byte stores and a (tiles, images) grid 3.2 / 1.3 / 1.3 TB/s at 640 x 480 x 3, 400 x 300 x 3
// and 1920 x 1080 x 1, as it stands 4.0 / 3.5 / 4.8.
//
// LDS layout: grey byte (r, c) at r*64 + 16*(r >> 4) + c -- a 64-byte pitch with each band of 16 rows skewed by one
// 16-byte slot.  At gather step j a wave reads rows 16k + j (k = lane & 3) of 16 consecutive columns (lane >> 2): dword
// 16*j + 4*k + (c >> 2) + const, i.e. 16 distinct banks (of 32), the 4 lanes of one dword broadcast: conflict-free
// (degree 1); the plain 64-byte pitch would put the four k on one bank (4-way).  The ds_write_b128 of the load phase
// cover consecutive 16-byte slots lane by lane: conflict-free.  The colour tile has a pitch of 64*CH bytes and a skew of
// 32 bytes per band: a 32-lane half (the conflict group of ds_read_b32) reads 8 columns of the four bands, CH = 4 dwords
// 8*k + c, CH = 3 the 6 dwords of 24 consecutive bytes at 8*k: conflict-free within the half, 2-way at most over a wave.
// Bound by HBM: w*h*CH bytes read, T*w*h written (+ T*w*h*CH with colour).
#include <cstdint>

#include "cbh_index.h"
#include "gray_px.h"

namespace {

constexpr int TILE = 64;

__device__ __forceinline__ unsigned byte_of(const unsigned* v, int i) { return (v[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// flag 8: out[y'][x'] = in[h-1-x'][y'], 16: in[x'][w-1-y'], 32: in[x'][y'], 64: in[h-1-x'][w-1-y']
__device__ __forceinline__ bool runs_back(int flag) { return flag == 8 || flag == 64; }    // x' falls as the source row grows
__device__ __forceinline__ bool rows_back(int flag) { return flag == 16 || flag == 64; }  // y' falls as the source column grows

// 16 pixels of NB bytes each (v: 4 * NB dwords) to d + first * NB, pixel j to position first + j, or, backwards,
// first + 15 - j; only the first np pixels when the chunk is ragged.  A whole chunk goes out in the widest stores its
// address allows: 16 bytes, 8, 4; a grey chunk at an odd address (odd h) as its first bytes up to a dword boundary, three
// dwords shifted into place (v_alignbyte_b32) and the bytes left over.
template <int NB>
__device__ __forceinline__ void put16(unsigned char* d, ptrdiff_t first, bool back, int np, const unsigned* v) {
  unsigned char* q = d + first * NB;
  if (np == 16) {
    unsigned o[4 * NB];  // the chunk in destination order
    if (!back) {
#pragma unroll
      for (int k = 0; k < 4 * NB; ++k) o[k] = v[k];
    } else if (NB == 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = __builtin_amdgcn_perm(0u, v[3 - k], 0x00010203u);
    } else if (NB == 4) {
#pragma unroll
      for (int k = 0; k < 16; ++k) o[k] = v[15 - k];
    } else {  // 3-byte pixels: constant byte moves
#pragma unroll
      for (int k = 0; k < 4 * NB; ++k) {
        unsigned x = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int b = 4 * k + j, p = b / NB, c = b - p * NB;
          x |= byte_of(v, (15 - p) * NB + c) << (8 * j);
        }
        o[k] = x;
      }
    }
    const unsigned a = (unsigned)(uintptr_t)q;
    if ((a & 15) == 0) {
#pragma unroll
      for (int k = 0; k < NB; ++k)
        reinterpret_cast<uint4*>(q)[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    } else if ((a & 7) == 0) {
#pragma unroll
      for (int k = 0; k < 2 * NB; ++k) reinterpret_cast<uint2*>(q)[k] = make_uint2(o[2 * k], o[2 * k + 1]);
    } else if ((a & 3) == 0) {
#pragma unroll
      for (int k = 0; k < 4 * NB; ++k) reinterpret_cast<unsigned*>(q)[k] = o[k];
    } else if (NB == 1) {
      const unsigned lead = 4 - (a & 3);  // 1..3 bytes up to the dword boundary
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if ((unsigned)j < lead) q[j] = (unsigned char)(o[0] >> (8 * j));
#pragma unroll
      for (int k = 0; k < 3; ++k) reinterpret_cast<unsigned*>(q + lead)[k] = __builtin_amdgcn_alignbyte(o[k + 1], o[k], lead);
      const unsigned rest = o[3] >> (8 * lead);  // the 4 - lead bytes behind the last whole dword
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if ((unsigned)j < 4 - lead) q[lead + 12 + j] = (unsigned char)(rest >> (8 * j));
    } else {
#pragma unroll
      for (int b = 0; b < 16 * NB; ++b) q[b] = (unsigned char)byte_of(o, b);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < np) {
        unsigned char* e = d + (first + (back ? 15 - j : j)) * NB;
#pragma unroll
        for (int c = 0; c < NB; ++c) e[c] = (unsigned char)byte_of(v, j * NB + c);
      }
  }
}

template <int CH, bool COLOR>
__global__ __launch_bounds__(256) void k_turn_views(const unsigned char* __restrict__ src, int w, int h, size_t row_stride,
                                                    size_t img_stride, int mask, int nt, unsigned tiles, int tiles_y,
                                                    unsigned char* __restrict__ gray /* n*nt planes of h*w */,
                                                    unsigned char* __restrict__ color /* n*nt images h*w*CH */) {
  constexpr bool CTILE = COLOR && CH != 1;  // (one channel: the colour image is the grey plane)
  __shared__ __attribute__((aligned(16))) unsigned char tg[TILE * TILE + 64];
  __shared__ __attribute__((aligned(16))) unsigned char tc[CTILE ? TILE * TILE * CH + 128 : 16];
  // Workgroups are dealt round-robin to the eight XCDs, each with an L2 of its own.  Workgroups that share an XCD (the
  // same blockIdx % 8) take consecutive tiles, down a column of tiles first: their 64-byte pieces of the destination
  // rows, and of the source rows, then meet in one L2 as whole lines.  (Bijective for any grid; a speed matter only.)
  const unsigned nwg = gridDim.x, per = nwg >> 3, odd = nwg & 7, grp = blockIdx.x & 7;
  const unsigned id = (grp < odd ? grp * (per + 1) : odd * (per + 1) + (grp - odd) * per) + (blockIdx.x >> 3);
  const unsigned t = id % tiles;
  const size_t img = id / tiles, plane = (size_t)w * h;
  const int tx = (int)(t / (unsigned)tiles_y), ty = (int)(t - (unsigned)tx * tiles_y);
  const int x0 = tx * TILE, y0 = ty * TILE, tid = threadIdx.x;
  {  // load: row r of the tile, columns 16q .. 16q + 15
    const int r = tid >> 2, q = tid & 3;
    const int y = y0 + r, x = x0 + 16 * q;
    const int np = y < h ? max(0, min(16, w - x)) : 0;
    unsigned px[4 * CH];
    if (np == 0) {
#pragma unroll
      for (int k = 0; k < 4 * CH; ++k) px[k] = 0;
    } else {
      const unsigned char* p = src + img * img_stride + (size_t)y * row_stride + (size_t)x * CH;
      if (np == 16 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int k = 0; k < CH; ++k) {
          const uint4 v = reinterpret_cast<const uint4*>(p)[k];
          px[4 * k] = v.x, px[4 * k + 1] = v.y, px[4 * k + 2] = v.z, px[4 * k + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4 * CH; ++k) px[k] = 0;
#pragma unroll
        for (int b = 0; b < 16 * CH; ++b)
          if (b < np * CH) px[b >> 2] |= (unsigned)p[b] << (8 * (b & 3));
      }
    }
    unsigned gw[4];
    if (CH == 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) gw[k] = px[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        unsigned v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int b = (4 * k + j) * CH;
          v |= (unsigned)cbh_gray_px((int)byte_of(px, b), (int)byte_of(px, b + 1), (int)byte_of(px, b + 2)) << (8 * j);
        }
        gw[k] = v;
      }
    }
    *reinterpret_cast<uint4*>(tg + r * TILE + 16 * (r >> 4) + 16 * q) = make_uint4(gw[0], gw[1], gw[2], gw[3]);
    if (CTILE) {
      uint4* d = reinterpret_cast<uint4*>(tc + r * TILE * CH + 32 * (r >> 4) + 16 * q * CH);
#pragma unroll
      for (int k = 0; k < CH; ++k) d[k] = make_uint4(px[4 * k], px[4 * k + 1], px[4 * k + 2], px[4 * k + 3]);
    }
  }
  __syncthreads();
  // store: source column x, source rows ys .. ys + 15 = 16 consecutive pixels of destination row x (or w - 1 - x)
  const int c = tid >> 2, k = tid & 3;
  const int x = x0 + c, ys = y0 + 16 * k;
  const int nr = min(16, h - ys);
  if (x >= w || nr <= 0) return;
  unsigned gw[4];  // grey of source rows ys + j, row j in byte j
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) v |= (unsigned)tg[(16 * k + 4 * i + j) * TILE + 16 * k + c] << (8 * j);
    gw[i] = v;
  }
  unsigned cw[CTILE ? 4 * CH : 1];  // the colour pixels of the same rows
  if (CTILE) {
    const unsigned char* t = tc + 16 * k * TILE * CH + 32 * k + c * CH;
    if (CH == 4) {
#pragma unroll
      for (int j = 0; j < 16; ++j) cw[j] = *reinterpret_cast<const unsigned*>(t + j * TILE * CH);
    } else {
#pragma unroll
      for (int i = 0; i < 4 * CH; ++i) {
        unsigned v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int b = 4 * i + j, p = b / CH, ch = b - p * CH;
          v |= (unsigned)t[p * TILE * CH + ch] << (8 * j);
        }
        cw[i] = v;
      }
    }
  }
  unsigned char* g0 = gray + img * (size_t)nt * plane;
  unsigned char* c0 = COLOR ? color + img * (size_t)nt * plane * CH : nullptr;
  int slot = 0;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int flag = 8 << f;
    if (!(mask & flag)) continue;
    const bool back = runs_back(flag);
    const size_t dy = (size_t)(rows_back(flag) ? w - 1 - x : x);
    // position of the chunk's first pixel in its destination row (a backward chunk's 16 pixels end at h - ys)
    const ptrdiff_t first = back ? (ptrdiff_t)h - ys - 16 : ys;
    put16<1>(g0 + (size_t)slot * plane + dy * (size_t)h, first, back, nr, gw);
    if (COLOR) {
      unsigned char* cd = c0 + ((size_t)slot * plane + dy * (size_t)h) * CH;
      if (CTILE) put16<CH>(cd, first, back, nr, cw);
      else put16<1>(cd, first, back, nr, gw);
    }
    ++slot;
  }
}

template <int CH>
void launch_turns(const unsigned char* src, size_t m, int w, int h, size_t row_stride, size_t img_stride, int mask, int nt,
                  unsigned tiles, unsigned char* gray, unsigned char* color, hipStream_t s) {
  const int tiles_y = (h + TILE - 1) / TILE;
  const dim3 grid(tiles * (unsigned)m);  // a workgroup per tile, the tiles of an image together
  if (color)
    hipLaunchKernelGGL((k_turn_views<CH, true>), grid, dim3(256), 0, s, src, w, h, row_stride, img_stride, mask, nt, tiles,
                       tiles_y, gray, color);
  else
    hipLaunchKernelGGL((k_turn_views<CH, false>), grid, dim3(256), 0, s, src, w, h, row_stride, img_stride, mask, nt, tiles,
                       tiles_y, gray, color);
}

}  // namespace

int cbh_turn_views_dev(const void* d_src, size_t n, int w, int h, size_t row_stride, size_t img_stride, int channels,
                       int turn_mask, void* d_gray, void* d_color, int device, void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (turn_mask <= 0 || (turn_mask & ~120)) return CBH_E_INVAL;
  if (n == 0) return CBH_OK;
  if (!d_src || !d_gray || w <= 0 || h <= 0 || (channels != 1 && channels != 3 && channels != 4) ||
      row_stride < (size_t)w * channels)
    return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  const int nt = __builtin_popcount((unsigned)turn_mask);
  unsigned char* color = (unsigned char*)d_color;
  const size_t plane = (size_t)w * h;
  const size_t tiles = (size_t)((w + TILE - 1) / TILE) * (size_t)((h + TILE - 1) / TILE);
  if (tiles > 0x7fffffffu) return CBH_E_OVERFLOW;
  const size_t per_launch = 0x7fffffffu / tiles;  // images per grid
  for (size_t i0 = 0; i0 < n; i0 += per_launch) {
    const size_t m = std::min<size_t>(per_launch, n - i0);
    const unsigned char* src = (const unsigned char*)d_src + i0 * img_stride;
    unsigned char* gr = (unsigned char*)d_gray + i0 * nt * plane;
    unsigned char* co = color ? color + i0 * nt * plane * channels : nullptr;
    if (channels == 1) launch_turns<1>(src, m, w, h, row_stride, img_stride, turn_mask, nt, (unsigned)tiles, gr, co, s);
    else if (channels == 3) launch_turns<3>(src, m, w, h, row_stride, img_stride, turn_mask, nt, (unsigned)tiles, gr, co, s);
    else launch_turns<4>(src, m, w, h, row_stride, img_stride, turn_mask, nt, (unsigned)tiles, gr, co, s);
  }
  CBH_HIP(hipGetLastError());
  if (!stream) CBH_HIP(hipStreamSynchronize(s));
  return CBH_OK;
}
