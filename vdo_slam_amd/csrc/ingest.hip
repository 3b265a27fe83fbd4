// Dataset ingest (example/vdo_slam.cc:104-131): a frame's instance-mask text, PNG scanlines and .flo payload decoded on the device
// into the four images FramePipeline::Step takes.  The host reads the files and inflates the PNGs (zlib, serial Huffman decoding);
// everything after that is here.
//
// Mask text.  LoadMask (host/DatasetIO.cc) is the definition, on every byte string.  Its tokenizer reduces to three facts that need no
// sequential state machine: (1) every maximal digit run is a token - a run is never swallowed, since the only character that swallows
// its successor is an active '-', and a digit after an active '-' starts a number; (2) the token is negative iff the run of '-' right in
// front of it has odd length (in a run of '-', the first, third, ... are active; each even one is swallowed by its predecessor; any
// other character in front of a '-' leaves it active); (3) whitespace and every other byte only separate runs.  So: a digit-run start
// is a byte that is a digit after a non-digit; its line is the number of '\n' in front of it, its column the number of starts in front
// of it on its line, its row the number of lines with a start in front of its line.  Those are prefix sums: per-thread chunk counts, a
// scan over the blocks, a scan over the lines; each start then converts its own digit run (value clamped like the host's once >= 1e8).
//
// PNG.  Sub / Avg / Paeth need the decoded left pixel and the row above, so one thread per row runs a diagonal wavefront: row y decodes
// pixel x at step x + y, right after row y-1 decoded it; the pixel goes from row to row through LDS.  One workgroup takes 1024 rows (a
// band); a taller image is decoded band by band, each band reading the row above it back from the scanline buffer.  The conversion
// (disparity -> float; colour -> ReadPNG's BGR(A) -> K2's grey) is fused into the step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"

using vdo::ctx_bind;
using vdo::set_error;

namespace {

constexpr int kThreads = 256, kChunk = 16, kBlockBytes = kThreads * kChunk;   // mask kernels: 16 bytes (or 16 lines) per thread
constexpr int kBand = 1024;                                                  // PNG: rows per workgroup
constexpr int kGroup = 8;                                                    // PNG: pixels per thread and step
constexpr int kMaxDim = 1 << 15;

__device__ __forceinline__ bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// exclusive scan over the block of an unsigned 64-bit value (NT threads, wave64); *total = the block's sum
template <int NT>
__device__ __forceinline__ unsigned long long block_scan(unsigned long long v, unsigned long long* lds, unsigned long long* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) lds[wave] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < NT / 64; ++w) { const unsigned long long t = lds[w]; lds[w] = s; s += t; }
    lds[NT / 64] = s;
  }
  __syncthreads();
  const unsigned long long r = lds[wave] + x - v;
  *total = lds[NT / 64];
  __syncthreads();
  return r;
}

// newline count in the high half, digit-run starts in the low half (a chunk holds at most 16 of either)
__device__ __forceinline__ unsigned long long chunk_counts(const uint8_t* __restrict__ t, int64_t base, uint8_t* c16) {
  const uint4 q = *(const uint4*)(t + base);
  std::memcpy(c16, &q, 16);
  bool prev_digit = base > 0 && is_digit(t[base - 1]);
  unsigned nl = 0, st = 0;
#pragma unroll
  for (int k = 0; k < kChunk; ++k) {
    const bool d = is_digit(c16[k]);
    st += d && !prev_digit;
    nl += c16[k] == '\n';
    prev_digit = d;
  }
  return ((unsigned long long)nl << 32) | st;
}

// per block of 4096 bytes: (newlines, starts)
__global__ __launch_bounds__(kThreads) void k_mask_count(const uint8_t* __restrict__ t, unsigned long long* __restrict__ blk) {
  __shared__ unsigned long long lds[kThreads / 64 + 1];
  uint8_t c[kChunk];
  const unsigned long long v = chunk_counts(t, (int64_t)blockIdx.x * kBlockBytes + threadIdx.x * kChunk, c);
  unsigned long long tot;
  block_scan<kThreads>(v, lds, &tot);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// one workgroup: exclusive scan of n values in place; total -> *total.  Optionally also sets up the line table of the mask
// (line_tok[0] = 0, line_tok[n_lines] = starts, meta = {n_lines, starts}).
__global__ __launch_bounds__(1024) void k_scan_single(unsigned long long* __restrict__ v, int64_t n, unsigned long long* __restrict__ total, int mask_meta,
                                                      int64_t* __restrict__ line_tok, int64_t* __restrict__ meta) {
  __shared__ unsigned long long lds[1024 / 64 + 1];
  unsigned long long carry = 0;
  for (int64_t b = 0; b < n; b += 1024) {
    const int64_t i = b + threadIdx.x;
    const unsigned long long x = i < n ? v[i] : 0;
    unsigned long long tot;
    const unsigned long long e = block_scan<1024>(x, lds, &tot);
    if (i < n) v[i] = carry + e;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    *total = carry;
    if (mask_meta) {
      const int64_t n_lines = (int64_t)(carry >> 32) + 1, starts = (int64_t)(carry & 0xffffffffull);
      meta[0] = n_lines; meta[1] = starts;
      line_tok[0] = 0; line_tok[n_lines] = starts;
    }
  }
}

// the start index of every line (line_tok[L + 1] = starts in front of the '\n' that ends line L); the thread's (line, start) offsets -> thr
__global__ __launch_bounds__(kThreads) void k_mask_lines(const uint8_t* __restrict__ t, const unsigned long long* __restrict__ blk, int64_t* __restrict__ line_tok,
                                                         unsigned long long* __restrict__ thr) {
  __shared__ unsigned long long lds[kThreads / 64 + 1];
  uint8_t c[kChunk];
  const int64_t base = (int64_t)blockIdx.x * kBlockBytes + threadIdx.x * kChunk;
  const unsigned long long v = chunk_counts(t, base, c);
  unsigned long long tot;
  const unsigned long long off = blk[blockIdx.x] + block_scan<kThreads>(v, lds, &tot);
  thr[(int64_t)blockIdx.x * kThreads + threadIdx.x] = off;
  int64_t L = (int64_t)(off >> 32), g = (int64_t)(off & 0xffffffffull);
  bool prev_digit = base > 0 && is_digit(t[base - 1]);
#pragma unroll
  for (int k = 0; k < kChunk; ++k) {
    const bool d = is_digit(c[k]);
    g += d && !prev_digit;
    prev_digit = d;
    if (c[k] == '\n') line_tok[++L] = g;
  }
}

// per block of 4096 lines: lines that hold a start
__global__ __launch_bounds__(kThreads) void k_line_count(const int64_t* __restrict__ line_tok, const int64_t* __restrict__ meta, unsigned long long* __restrict__ blk) {
  __shared__ unsigned long long lds[kThreads / 64 + 1];
  const int64_t n_lines = meta[0], L0 = (int64_t)blockIdx.x * kBlockBytes + threadIdx.x * kChunk;
  unsigned long long cnt = 0;
  for (int k = 0; k < kChunk; ++k) { const int64_t L = L0 + k; if (L < n_lines) cnt += line_tok[L + 1] > line_tok[L]; }
  unsigned long long tot;
  block_scan<kThreads>(cnt, lds, &tot);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// row of every line = lines with a start in front of it
__global__ __launch_bounds__(kThreads) void k_line_rows(const int64_t* __restrict__ line_tok, const int64_t* __restrict__ meta, const unsigned long long* __restrict__ blk,
                                                        int64_t* __restrict__ line_row) {
  __shared__ unsigned long long lds[kThreads / 64 + 1];
  const int64_t n_lines = meta[0], L0 = (int64_t)blockIdx.x * kBlockBytes + threadIdx.x * kChunk;
  unsigned long long cnt = 0;
  for (int k = 0; k < kChunk; ++k) { const int64_t L = L0 + k; if (L < n_lines) cnt += line_tok[L + 1] > line_tok[L]; }
  unsigned long long tot;
  int64_t r = (int64_t)(blk[blockIdx.x] + block_scan<kThreads>(cnt, lds, &tot));
  for (int k = 0; k < kChunk; ++k) {
    const int64_t L = L0 + k;
    if (L < n_lines) { line_row[L] = r; r += line_tok[L + 1] > line_tok[L]; }
  }
}

// every digit-run start writes its token (the output was zeroed first)
__global__ __launch_bounds__(kThreads) void k_mask_emit(const uint8_t* __restrict__ t, int64_t n, const unsigned long long* __restrict__ thr, const int64_t* __restrict__ line_tok,
                                                        const int64_t* __restrict__ line_row, int rows, int cols, int32_t* __restrict__ out) {
  const int64_t base = (int64_t)blockIdx.x * kBlockBytes + threadIdx.x * kChunk;
  const uint4 q = *(const uint4*)(t + base);
  uint8_t c[kChunk];
  std::memcpy(c, &q, 16);
  const unsigned long long off = thr[(int64_t)blockIdx.x * kThreads + threadIdx.x];
  int64_t L = (int64_t)(off >> 32), g = (int64_t)(off & 0xffffffffull);
  bool prev_digit = base > 0 && is_digit(t[base - 1]);
  for (int k = 0; k < kChunk; ++k) {
    const bool d = is_digit(c[k]);
    if (d && !prev_digit) {
      const int64_t row = line_row[L], col = g - line_tok[L];
      if (row < rows && col < cols) {
        int64_t i = base + k;
        int v = 0;
        while (i < n && is_digit(t[i]) && v < 100000000) { v = v * 10 + (t[i] - '0'); ++i; }      // (digits past the clamp change nothing)
        int64_t j = base + k - 1, minus = 0;
        while (j >= 0 && t[j] == '-') { ++minus; --j; }
        out[row * cols + col] = (minus & 1) ? -v : v;
      }
      ++g;
    }
    prev_digit = d;
    if (c[k] == '\n') ++L;
  }
}

// ---- PNG
// device layout of the scanlines: row y at y * dev_pitch, its filter byte at +15, its pixels from +16 (16-byte aligned), room for whole groups
__host__ __device__ inline int64_t dev_pitch(int W, int bpp) { return 16 + ((((int64_t)(W + kGroup - 1) / kGroup) * kGroup * bpp + 15) / 16) * 16; }

// linear scanlines (as inflated) -> the device layout above
__global__ __launch_bounds__(256) void k_repitch(const uint8_t* __restrict__ lin, int64_t src_pitch, int H, uint8_t* __restrict__ dst, int64_t dst_pitch) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= src_pitch * H) return;
  const int64_t y = i / src_pitch, x = i - y * src_pitch;
  dst[y * dst_pitch + 15 + x] = lin[i];
}

template <int BPP>
__device__ __forceinline__ uint32_t load_px(const uint8_t* __restrict__ p) {
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < BPP; ++k) v |= (uint32_t)p[k] << (8 * k);
  return v;
}

__device__ __forceinline__ int unfilter_byte(int ft, int x, int a, int b, int c) {
  int pred;
  switch (ft) {
    case 1: pred = a; break;
    case 2: pred = b; break;
    case 3: pred = (a + b) >> 1; break;
    case 4: { const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c); pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); break; }
    default: pred = 0;
  }
  return (x + pred) & 255;
}

// MODE 0: grey -> float (ReadPNG(.., as_float = true): 16-bit samples are big-endian); MODE 1: -> grey u8 (ReadPNG's BGR(A) through K2).
// Thread r decodes the kGroup pixels of group j at step j + r: row r-1 decoded the same group (the pixels above) one step earlier.
template <int BPP, int MODE>
__global__ __launch_bounds__(kBand) void k_png_band(uint8_t* __restrict__ scan, int W, int H, int y0, int rgb_order, void* __restrict__ out) {
  __shared__ uint32_t xch[2][kGroup][kBand];
  const int r = threadIdx.x, y = y0 + r;
  const int nrows = min(kBand, H - y0);
  const int64_t pitch = dev_pitch(W, BPP);
  const bool active = r < nrows;
  uint8_t* row = scan + (int64_t)(active ? y : y0) * pitch;
  const uint8_t* above = y0 > 0 ? scan + (int64_t)(y0 - 1) * pitch + 16 : nullptr;     // band > 0: the row above, decoded in place by the last band
  const int ft = active ? row[15] : 0;
  const bool keep_raw = active && r == nrows - 1 && y + 1 < H;                          // the band's last row stays decoded in place for the next band
  const int ngroups = (W + kGroup - 1) / kGroup;
  uint2 nxt[BPP];
  auto load_group = [&](int j) {
#pragma unroll
    for (int i = 0; i < BPP; ++i) nxt[i] = ((const uint2*)(row + 16 + (int64_t)j * kGroup * BPP))[i];      // the group's kGroup * BPP bytes, 8-byte aligned
  };
  if (active) load_group(0);
  uint32_t left = 0, upleft = 0;
  const int steps = ngroups + nrows - 1;
  for (int t = 0; t < steps; ++t) {
    const int j = t - r;
    if (active && j >= 0 && j < ngroups) {
      uint32_t raw[kGroup], up[kGroup];
      {
        uint8_t bytes[kGroup * BPP];
        std::memcpy(bytes, nxt, sizeof(bytes));
#pragma unroll
        for (int k = 0; k < kGroup; ++k) {
          raw[k] = 0;
#pragma unroll
          for (int b = 0; b < BPP; ++b) raw[k] |= (uint32_t)bytes[k * BPP + b] << (8 * b);
        }
      }
      if (j + 1 < ngroups) load_group(j + 1);                                           // (in flight over this step and its barrier)
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        const int x = kGroup * j + k;
        up[k] = r > 0 ? xch[(t - 1) & 1][k][r - 1] : (above && x < W ? load_px<BPP>(above + (int64_t)x * BPP) : 0u);
      }
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        const int x = kGroup * j + k;
        if (x >= W) break;
        uint32_t px = 0;
#pragma unroll
        for (int b = 0; b < BPP; ++b)
          px |= (uint32_t)unfilter_byte(ft, (raw[k] >> (8 * b)) & 255, (left >> (8 * b)) & 255, (up[k] >> (8 * b)) & 255, (upleft >> (8 * b)) & 255) << (8 * b);
        xch[t & 1][k][r] = px;
        const int64_t o = (int64_t)y * W + x;
        if (MODE == 0) ((float*)out)[o] = BPP == 2 ? (float)(((px & 255) << 8) | (px >> 8)) : (float)(px & 255);
        else if (BPP == 1) ((uint8_t*)out)[o] = (uint8_t)px;
        else {
          // ReadPNG hands K2 the pixel in BGR order (cv::imread): p[0] = file B, p[1] = G, p[2] = file R; K2 = k_rgb2gray (orb.hip)
          const int p0 = (px >> 16) & 255, p1 = (px >> 8) & 255, p2 = px & 255;
          const int R = rgb_order ? p0 : p2, G = p1, B = rgb_order ? p2 : p0;
          ((uint8_t*)out)[o] = (uint8_t)((R * 4899 + G * 9617 + B * 1868 + 8192) >> 14);
        }
        if (keep_raw)
#pragma unroll
          for (int b = 0; b < BPP; ++b) row[16 + (int64_t)x * BPP + b] = (uint8_t)(px >> (8 * b));
        left = px; upleft = up[k];
      }
    }
    __syncthreads();
  }
}

template <int BPP, int MODE>
void launch_png(uint8_t* scan, int W, int H, int rgb_order, void* out, hipStream_t s) {
  for (int y0 = 0; y0 < H; y0 += kBand) hipLaunchKernelGGL((k_png_band<BPP, MODE>), dim3(1), dim3(kBand), 0, s, scan, W, H, y0, rgb_order, out);
}

}  // namespace

struct vdo_ingest {
  vdo_ctx* ctx = nullptr;
  int w = 0, h = 0;
  // pinned staging per input kind + its size
  void* h_buf[4] = {nullptr, nullptr, nullptr, nullptr}; size_t h_cap[4] = {0, 0, 0, 0};
  // device: mask text (padded to whole blocks), scanlines of the two PNGs, the mask scan tables
  uint8_t* d_text = nullptr; size_t text_cap = 0;
  uint8_t* d_scan[2] = {nullptr, nullptr}; size_t scan_cap[2] = {0, 0};
  uint8_t* d_lin[2] = {nullptr, nullptr}; size_t lin_cap[2] = {0, 0};       // the scanlines as uploaded (one linear copy), before k_repitch
  unsigned long long *d_blk = nullptr, *d_thr = nullptr, *d_tot = nullptr; int64_t *d_line_tok = nullptr, *d_line_row = nullptr, *d_meta = nullptr;
  size_t blk_cap = 0, thr_cap = 0, lt_cap = 0, lr_cap = 0;
  int64_t* h_meta = nullptr;                 // pinned: n_lines, starts
  // outputs owned by the handle (vdo_ingest_device_outputs)
  uint8_t* d_gray = nullptr; float *d_depth = nullptr, *d_flow = nullptr; int32_t* d_mask = nullptr;
  hipEvent_t ev[6] = {};
  hipStream_t side = nullptr;                // the colour PNG's wavefront next to the disparity PNG's (one workgroup each)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  double ms[3] = {0, 0, 0};
};

namespace {
int grow_device(void** p, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return VDO_OK;
  if (*p) hipFree(*p);
  *p = nullptr; *cap = 0;
  const size_t want = bytes + bytes / 4;
  if (hipMalloc(p, want) != hipSuccess) { *p = nullptr; return set_error(VDO_ERR_OOM, "vdo_ingest: hipMalloc(%zu) failed", want); }
  *cap = want;
  return VDO_OK;
}

int check_png(const vdo_png_scanlines* p, int W, int H, bool depth, const char* kind) {
  if (!p->data) return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: %s PNG: null scanlines", kind);
  if (p->width != W || p->height != H)
    return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: %s PNG is %dx%d, the handle %dx%d", kind, p->width, p->height, W, H);
  if (depth ? !(p->channels == 1 && (p->bit_depth == 8 || p->bit_depth == 16)) : !(p->bit_depth == 8 && (p->channels == 1 || p->channels == 3 || p->channels == 4)))
    return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: %s PNG: %d-bit with %d channel(s) is not supported (%s)", kind, p->bit_depth, p->channels,
                     depth ? "8/16-bit grey" : "8-bit grey / RGB / RGBA");
  const int64_t pitch = (int64_t)W * p->channels * (p->bit_depth / 8) + 1;
  if (p->bytes != pitch * H)
    return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: %s PNG: %lld bytes of scanlines, %lld expected", kind, (long long)p->bytes, (long long)(pitch * H));
  for (int y = 0; y < H; ++y)
    if (p->data[(int64_t)y * pitch] > 4) return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: %s PNG: filter type %d in row %d", kind, p->data[(int64_t)y * pitch], y);
  return VDO_OK;
}
}  // namespace

extern "C" int vdo_ingest_create(vdo_ctx* ctx, int width, int height, vdo_ingest** out) {
  if (!ctx || !out || width <= 0 || height <= 0 || width > kMaxDim || height > kMaxDim) return set_error(VDO_ERR_INVALID, "vdo_ingest_create: bad argument");
  int rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  vdo_ingest* h = new vdo_ingest();
  h->ctx = ctx; h->w = width; h->h = height;
  const size_t n = (size_t)width * height;
  bool ok = hipMalloc((void**)&h->d_gray, n) == hipSuccess && hipMalloc((void**)&h->d_depth, 4 * n) == hipSuccess &&
            hipMalloc((void**)&h->d_flow, 8 * n) == hipSuccess && hipMalloc((void**)&h->d_mask, 4 * n) == hipSuccess &&
            hipMalloc((void**)&h->d_meta, 16) == hipSuccess && hipMalloc((void**)&h->d_tot, 16) == hipSuccess &&
            hipHostMalloc((void**)&h->h_meta, 16) == hipSuccess;
  for (hipEvent_t& e : h->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  ok = ok && hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) == hipSuccess &&
       hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) == hipSuccess;
  if (!ok) { vdo_ingest_destroy(h); return set_error(VDO_ERR_OOM, "vdo_ingest_create: allocation failed"); }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_ingest_destroy(vdo_ingest* h) {
  if (!h) return VDO_OK;
  hipSetDevice(h->ctx->device);
  hipStreamSynchronize(h->ctx->stream);
  for (void* p : h->h_buf) if (p) hipHostFree(p);
  if (h->h_meta) hipHostFree(h->h_meta);
  for (void* p : {(void*)h->d_lin[0], (void*)h->d_lin[1], (void*)h->d_text, (void*)h->d_scan[0], (void*)h->d_scan[1], (void*)h->d_blk, (void*)h->d_thr, (void*)h->d_tot, (void*)h->d_line_tok, (void*)h->d_line_row,
                  (void*)h->d_meta, (void*)h->d_gray, (void*)h->d_depth, (void*)h->d_flow, (void*)h->d_mask})
    if (p) hipFree(p);
  for (hipEvent_t e : h->ev) if (e) hipEventDestroy(e);
  for (hipEvent_t e : {h->ev_fork, h->ev_join}) if (e) hipEventDestroy(e);
  if (h->side) hipStreamDestroy(h->side);
  delete h;
  return VDO_OK;
}

extern "C" int vdo_ingest_host_buffer(vdo_ingest* h, int which, int64_t bytes, void** ptr) {
  if (!h || !ptr || which < 0 || which > 3 || bytes < 0) return set_error(VDO_ERR_INVALID, "vdo_ingest_host_buffer: bad argument");
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  if ((size_t)bytes > h->h_cap[which] || !h->h_buf[which]) {
    hipStreamSynchronize(h->ctx->stream);
    if (h->h_buf[which]) hipHostFree(h->h_buf[which]);
    h->h_buf[which] = nullptr; h->h_cap[which] = 0;
    const size_t want = (size_t)bytes + (size_t)bytes / 4 + 4096;
    if (hipHostMalloc(&h->h_buf[which], want) != hipSuccess) { h->h_buf[which] = nullptr; return set_error(VDO_ERR_OOM, "vdo_ingest_host_buffer: hipHostMalloc(%zu) failed", want); }
    h->h_cap[which] = want;
  }
  *ptr = h->h_buf[which];
  return VDO_OK;
}

extern "C" int vdo_ingest_device_outputs(vdo_ingest* h, uint8_t** gray, float** depth_raw, float** flow, int32_t** mask) {
  if (!h) return set_error(VDO_ERR_INVALID, "vdo_ingest_device_outputs: null handle");
  if (gray) *gray = h->d_gray;
  if (depth_raw) *depth_raw = h->d_depth;
  if (flow) *flow = h->d_flow;
  if (mask) *mask = h->d_mask;
  return VDO_OK;
}

extern "C" int vdo_ingest_frame(vdo_ingest* h, const char* mask_text, int64_t mask_bytes, const void* flo, int64_t flo_bytes, const vdo_png_scanlines* depth,
                                const vdo_png_scanlines* color, int rgb_order, uint8_t* gray, float* depth_raw, float* flow, int32_t* mask) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!h) return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: null handle");
  const int W = h->w, H = h->h;
  const int64_t np = (int64_t)W * H;
  // ---- everything the host can see is checked before any device work
  if ((gray && !color) || (depth_raw && !depth) || (flow && !flo) || (mask && !mask_text)) return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: an output without its input");
  if (mask && mask_bytes <= 0) return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: mask text: no row (empty file)");
  if (flow) {
    float magic; int32_t fw, fh;
    if (flo_bytes < 12) return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: .flo: %lld bytes, shorter than the header", (long long)flo_bytes);
    std::memcpy(&magic, flo, 4); std::memcpy(&fw, (const char*)flo + 4, 4); std::memcpy(&fh, (const char*)flo + 8, 4);
    if (magic != 202021.25f) return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: .flo: bad magic");
    if (fw != W || fh != H) return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: .flo is %dx%d, the handle %dx%d", fw, fh, W, H);
    if (flo_bytes < 12 + 8 * np) return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: .flo: truncated (%lld bytes, %lld expected)", (long long)flo_bytes, (long long)(12 + 8 * np));
  }
  int rc;
  if (depth_raw && (rc = check_png(depth, W, H, true, "depth")) != VDO_OK) return rc;
  if (gray && (rc = check_png(color, W, H, false, "colour")) != VDO_OK) return rc;
  if ((rc = ctx_bind(h->ctx)) != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  // ---- phase 1: uploads + the mask's scans (into the handle's own buffers); the host learns whether the text has a row
  if (mask && mask_bytes >= (int64_t)1 << 31) return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: mask text: %lld bytes (2 GiB at most)", (long long)mask_bytes);
  const int64_t nb = mask ? (mask_bytes + kBlockBytes - 1) / kBlockBytes : 0;           // blocks of text
  const int64_t nlb = mask ? (mask_bytes + 2 + kBlockBytes - 1) / kBlockBytes : 0;      // blocks of lines (n_lines <= bytes + 1)
  if (mask) {
    if ((rc = grow_device((void**)&h->d_text, &h->text_cap, (size_t)(nb * kBlockBytes))) != VDO_OK ||
        (rc = grow_device((void**)&h->d_blk, &h->blk_cap, 8 * (size_t)std::max(nb, nlb))) != VDO_OK ||
        (rc = grow_device((void**)&h->d_thr, &h->thr_cap, 8 * (size_t)(nb * kThreads))) != VDO_OK ||
        (rc = grow_device((void**)&h->d_line_tok, &h->lt_cap, 8 * (size_t)(mask_bytes + 2))) != VDO_OK ||
        (rc = grow_device((void**)&h->d_line_row, &h->lr_cap, 8 * (size_t)(mask_bytes + 1))) != VDO_OK)
      return rc;
  }
  const int bpp_d = depth_raw ? depth->channels * depth->bit_depth / 8 : 0, bpp_c = gray ? color->channels : 0;
  if (depth_raw && (rc = grow_device((void**)&h->d_scan[0], &h->scan_cap[0], (size_t)(dev_pitch(W, bpp_d) * H))) != VDO_OK) return rc;
  if (gray && (rc = grow_device((void**)&h->d_scan[1], &h->scan_cap[1], (size_t)(dev_pitch(W, bpp_c) * H))) != VDO_OK) return rc;
  if (depth_raw && (rc = grow_device((void**)&h->d_lin[0], &h->lin_cap[0], (size_t)depth->bytes)) != VDO_OK) return rc;
  if (gray && (rc = grow_device((void**)&h->d_lin[1], &h->lin_cap[1], (size_t)color->bytes)) != VDO_OK) return rc;
  hipEventRecord(h->ev[0], s);
  if (mask) {
    hipMemcpyAsync(h->d_text, mask_text, (size_t)mask_bytes, hipMemcpyHostToDevice, s);
    if (nb * kBlockBytes > mask_bytes) hipMemsetAsync(h->d_text + mask_bytes, 0, (size_t)(nb * kBlockBytes - mask_bytes), s);   // (a NUL byte only separates tokens)
  }
  // (one linear copy each; k_repitch then starts every row's pixels 16-byte aligned, so a thread reads its group with 8-byte loads)
  if (depth_raw) hipMemcpyAsync(h->d_lin[0], depth->data, (size_t)depth->bytes, hipMemcpyHostToDevice, s);
  if (gray) hipMemcpyAsync(h->d_lin[1], color->data, (size_t)color->bytes, hipMemcpyHostToDevice, s);
  hipEventRecord(h->ev[1], s);
  if (depth_raw)
    hipLaunchKernelGGL(k_repitch, dim3((unsigned)((depth->bytes + 255) / 256)), dim3(256), 0, s, (const uint8_t*)h->d_lin[0], (int64_t)W * bpp_d + 1, H, h->d_scan[0], dev_pitch(W, bpp_d));
  if (gray)
    hipLaunchKernelGGL(k_repitch, dim3((unsigned)((color->bytes + 255) / 256)), dim3(256), 0, s, (const uint8_t*)h->d_lin[1], (int64_t)W * bpp_c + 1, H, h->d_scan[1], dev_pitch(W, bpp_c));
  if (mask) {
    hipLaunchKernelGGL(k_mask_count, dim3((unsigned)nb), dim3(kThreads), 0, s, (const uint8_t*)h->d_text, h->d_blk);
    hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, s, h->d_blk, nb, h->d_tot, 1, h->d_line_tok, h->d_meta);
    hipLaunchKernelGGL(k_mask_lines, dim3((unsigned)nb), dim3(kThreads), 0, s, (const uint8_t*)h->d_text, (const unsigned long long*)h->d_blk, h->d_line_tok, h->d_thr);
    hipLaunchKernelGGL(k_line_count, dim3((unsigned)nlb), dim3(kThreads), 0, s, (const int64_t*)h->d_line_tok, (const int64_t*)h->d_meta, h->d_blk);
    hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, s, h->d_blk, nlb, h->d_tot + 1, 0, nullptr, nullptr);
    hipLaunchKernelGGL(k_line_rows, dim3((unsigned)nlb), dim3(kThreads), 0, s, (const int64_t*)h->d_line_tok, (const int64_t*)h->d_meta, (const unsigned long long*)h->d_blk,
                       h->d_line_row);
    hipMemcpyAsync(h->h_meta, h->d_meta, 16, hipMemcpyDeviceToHost, s);
  }
  hipEventRecord(h->ev[2], s);
  hipError_t e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "vdo_ingest_frame: %s", hipGetErrorString(e));
  if (mask && h->h_meta[1] == 0) return set_error(VDO_ERR_INVALID, "vdo_ingest_frame: mask text: no row (no integer in %lld bytes)", (long long)mask_bytes);
  // ---- phase 2: the outputs
  hipEventRecord(h->ev[3], s);
  if (gray) {                                        // (on the side stream: the two wavefronts are one workgroup each)
    hipEventRecord(h->ev_fork, s);
    hipStreamWaitEvent(h->side, h->ev_fork, 0);
    if (color->channels == 1) launch_png<1, 1>(h->d_scan[1], W, H, rgb_order, gray, h->side);
    else if (color->channels == 3) launch_png<3, 1>(h->d_scan[1], W, H, rgb_order, gray, h->side);
    else launch_png<4, 1>(h->d_scan[1], W, H, rgb_order, gray, h->side);
  }
  if (depth_raw) {
    if (depth->bit_depth == 16) launch_png<2, 0>(h->d_scan[0], W, H, 0, depth_raw, s);
    else launch_png<1, 0>(h->d_scan[0], W, H, 0, depth_raw, s);
  }
  if (mask) {
    hipMemsetAsync(mask, 0, (size_t)(4 * np), s);                                       // cells the text does not reach
    hipLaunchKernelGGL(k_mask_emit, dim3((unsigned)nb), dim3(kThreads), 0, s, (const uint8_t*)h->d_text, mask_bytes, (const unsigned long long*)h->d_thr,
                       (const int64_t*)h->d_line_tok, (const int64_t*)h->d_line_row, H, W, mask);
  }
  if (gray) {
    hipEventRecord(h->ev_join, h->side);
    hipStreamWaitEvent(s, h->ev_join, 0);
  }
  hipEventRecord(h->ev[4], s);
  if (flow) hipMemcpyAsync(flow, (const char*)flo + 12, (size_t)(8 * np), hipMemcpyHostToDevice, s);
  hipEventRecord(h->ev[5], s);
  e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "vdo_ingest_frame: %s", hipGetErrorString(e));
  float a = 0, b = 0, c = 0, d = 0;
  hipEventElapsedTime(&a, h->ev[0], h->ev[2]); hipEventElapsedTime(&b, h->ev[3], h->ev[5]);
  hipEventElapsedTime(&c, h->ev[1], h->ev[2]); hipEventElapsedTime(&d, h->ev[3], h->ev[4]);
  h->ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  h->ms[1] = a + b; h->ms[2] = c + d;
  return VDO_OK;
}

extern "C" int vdo_ingest_last_timing(vdo_ingest* h, double ms[3]) {
  if (!h || !ms) return set_error(VDO_ERR_INVALID, "vdo_ingest_last_timing: bad argument");
  for (int k = 0; k < 3; ++k) ms[k] = h->ms[k];
  return VDO_OK;
}
