// GPU-side training-input transform: the reference's loader pipeline
// Resize(size) -> RandomHorizontalFlip -> ToTensor -> Normalize(0.5, 0.5)
// (src/data_loaders.py:66-80, 100-112) as one HBM-bound kernel from uint8 HWC images to the f32
// NCHW batch the model consumes. Resize is Pillow's 8-bit fixed-point bilinear resampling (the
// library under torchvision's PIL path; restated and pinned in oracle/preprocess.py), reproduced
// bit-exactly: coefficients in double without FMA contraction, horizontal pass clipped to uint8,
// then the vertical pass. Ratios up to 4x (at most 9 taps per axis) run the tiled two-pass LDS
// kernel, which computes each column's and row's weights once per block; larger ratios run the
// generic kernel (one thread per output pixel, every weight recomputed - deterministically, so the
// normalising sum and each weight still match Pillow).
// vit_preprocess_u8_gather is the same transform fed from a resident dataset: output image b reads source
// image index[b] (HWC or planar CHW, as CIFAR's files store it) and its label travels with it, so a training
// step's input is one launch with no index_select copy. Both kernels serve both entries; the layouts differ
// only in Px<LAYOUT>, the pixel fetch.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;

struct Axis {
  double scale, support, ss;
  int in_size;
};

__host__ __device__ inline Axis make_axis(int in_size, int out_size) {
  Axis a;
  a.scale = (double)in_size / (double)out_size;
  const double filterscale = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = 1.0 * filterscale;
  a.ss = 1.0 / filterscale;
  a.in_size = in_size;
  return a;
}

__device__ inline double tri(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

// Pillow precompute_coeffs for output index xx: first tap, tap count, centre and weight sum.
__device__ inline void taps(const Axis& a, int xx, int& xmin, int& cnt, double& center, double& ww) {
#pragma clang fp contract(off)
  center = (xx + 0.5) * a.scale;
  xmin = (int)(center - a.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + a.support + 0.5);
  if (xmax > a.in_size) xmax = a.in_size;
  cnt = xmax - xmin;
  ww = 0.0;
  for (int x = 0; x < cnt; ++x) ww += tri((x + xmin - center + 0.5) * a.ss);
}

// normalize_coeffs_8bpp: fixed-point weight of tap x
__device__ inline int coeff(const Axis& a, int x, int xmin, double center, double ww) {
#pragma clang fp contract(off)
  double w = tri((x + xmin - center + 0.5) * a.ss);
  if (ww != 0.0) w = w / ww;
  return w < 0 ? (int)(-0.5 + w * (double)(1 << kPrecisionBits)) : (int)(0.5 + w * (double)(1 << kPrecisionBits));
}

__device__ inline int clip8(int v) {
  if (v >= (1 << kPrecisionBits << 8)) return 255;
  if (v <= 0) return 0;
  return v >> kPrecisionBits;
}

struct PrepArgs {
  const uint8_t* in;
  long in_bs;  // bytes between images
  int H, W, oh, ow, B;
  const uint8_t* flips;
  float mean[3], stdv[3];
  float* out;
  // gather (vit_preprocess_u8_gather): output image b reads source image index[b]; NULL = image b
  const int64_t* index;
  long n_images;
  const int64_t* labels_in;
  int64_t* labels_out;
};

constexpr int kLayoutHWC = 0, kLayoutCHW = 1;

// The pixel fetch, the only per-layout code: channel c of the pixel k columns right of q is q[k * kStep + c * cs].
// HWC interleaves the channels (step 3, cs 1); planar CHW is plane[c][row * W + col] (step 1, cs H * W). Byte
// loads only: nothing is assumed about alignment (W may be odd).
template <int LAYOUT>
struct Px {
  static constexpr int kStep = LAYOUT == kLayoutHWC ? 3 : 1;
  __device__ static inline long chan_stride(const PrepArgs& p) { return LAYOUT == kLayoutHWC ? 1 : (long)p.H * p.W; }
  __device__ static inline const uint8_t* at(const uint8_t* img, const PrepArgs& p, int row, int col) {
    return img + ((long)row * p.W + col) * kStep;
  }
};

// Source image of output image b: b itself without an index, else index[b], or -1 when that is outside
// [0, n_images) - such an image is never read through: its output is NaN and its label -1 (the rule
// vit_cross_entropy has for a bad label).
__device__ inline long source_image(const PrepArgs& p, int b) {
  if (!p.index) return b;
  const long s = p.index[b];
  return s >= 0 && s < p.n_images ? s : -1;
}

__device__ inline void gather_label(const PrepArgs& p, int b, long src) {
  if (p.labels_in && p.labels_out) p.labels_out[b] = src < 0 ? -1 : p.labels_in[src];
}

template <int LAYOUT>
__global__ void __launch_bounds__(256) preprocess_kernel(PrepArgs p) {
#pragma clang fp contract(off)
  const Axis ax = make_axis(p.W, p.ow), ay = make_axis(p.H, p.oh);
  const long plane = (long)p.oh * p.ow;
  const long total = (long)p.B * plane;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / plane);
    const int rem = (int)(i - (long)b * plane);
    const int y = rem / p.ow, x = rem - y * p.ow;
    const long srci = source_image(p, b);
    if (rem == 0) gather_label(p, b, srci);
    float* o = p.out + (long)b * 3 * plane + rem;
    if (srci < 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * plane] = __builtin_nanf("");
      continue;
    }
    const int xs = (p.flips && p.flips[b]) ? p.ow - 1 - x : x;  // the flip mirrors the resized image
    int xmin, xcnt, ymin, ycnt;
    double xc, xw, yc, yw;
    taps(ax, xs, xmin, xcnt, xc, xw);
    taps(ay, y, ymin, ycnt, yc, yw);
    const uint8_t* img = p.in + srci * p.in_bs;
    const long cs = Px<LAYOUT>::chan_stride(p);
    int acc0 = 1 << (kPrecisionBits - 1), acc1 = acc0, acc2 = acc0;
    for (int j = 0; j < ycnt; ++j) {
      const uint8_t* row = Px<LAYOUT>::at(img, p, ymin + j, xmin);
      int h0 = 1 << (kPrecisionBits - 1), h1 = h0, h2 = h0;
      for (int k = 0; k < xcnt; ++k) {
        const int c = coeff(ax, k, xmin, xc, xw);
        h0 += row[Px<LAYOUT>::kStep * k] * c;
        h1 += row[Px<LAYOUT>::kStep * k + cs] * c;
        h2 += row[Px<LAYOUT>::kStep * k + 2 * cs] * c;
      }
      const int cy = coeff(ay, j, ymin, yc, yw);
      acc0 += clip8(h0) * cy;
      acc1 += clip8(h1) * cy;
      acc2 += clip8(h2) * cy;
    }
    const int v[3] = {clip8(acc0), clip8(acc1), clip8(acc2)};
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = ((float)v[c] / 255.0f - p.mean[c]) / p.stdv[c];
  }
}

// Fast path (every axis with at most KMAX <= 9 taps, i.e. ratios up to 4x): a block owns 64 output
// columns x 32 output rows of one image and runs Pillow's two passes through LDS. Pass 1: the
// horizontal pass over the band of input rows those 32 output rows read (at most 31 * 4 + 1 + 9
// rows), each thread one output column with its weights in registers (computed once), results
// clipped to 8 bits into LDS. Pass 2: the vertical pass for the 32 rows from LDS with the row
// weights (computed once per block by 32 threads). Every input pixel is gathered once per block
// instead of once per output row that uses it.
constexpr int kColsPerBlock = 64, kRowsPerBlock = 32, kRowLanes = 4, kBandMax = 31 * 4 + 1 + 9;

template <int KMAX, int LAYOUT>
__global__ void __launch_bounds__(kColsPerBlock* kRowLanes) preprocess_tiled_kernel(PrepArgs p) {
#pragma clang fp contract(off)
  __shared__ int s_ky[kRowsPerBlock][KMAX];
  __shared__ int s_ymin[kRowsPerBlock], s_ycnt[kRowsPerBlock];
  __shared__ uint32_t s_h[kBandMax][kColsPerBlock];  // horizontal pass, (r, g, b) bytes
  const Axis ax = make_axis(p.W, p.ow), ay = make_axis(p.H, p.oh);
  const int b = blockIdx.z;
  const int y0 = blockIdx.y * kRowsPerBlock;
  const int rows = p.oh - y0 < kRowsPerBlock ? p.oh - y0 : kRowsPerBlock;
  const int tid = threadIdx.y * kColsPerBlock + threadIdx.x;
  const long srci = source_image(p, b);  // the same for the whole block
  if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) gather_label(p, b, srci);
  if (srci < 0) {
    const int xo = blockIdx.x * kColsPerBlock + threadIdx.x;
    if (xo < p.ow) {
      const long pl = (long)p.oh * p.ow;
      float* o = p.out + (long)b * 3 * pl + xo;
      for (int r = threadIdx.y; r < rows; r += kRowLanes)
        for (int c = 0; c < 3; ++c) o[c * pl + (long)(y0 + r) * p.ow] = __builtin_nanf("");
    }
    return;
  }
  if (tid < rows) {
    int ymin, ycnt;
    double yc, yw;
    taps(ay, y0 + tid, ymin, ycnt, yc, yw);
    s_ymin[tid] = ymin;
    s_ycnt[tid] = ycnt;
    for (int j = 0; j < KMAX; ++j) s_ky[tid][j] = j < ycnt ? coeff(ay, j, ymin, yc, yw) : 0;
  }
  const int x = blockIdx.x * kColsPerBlock + threadIdx.x;
  const bool live = x < p.ow;
  const int xs = live && p.flips && p.flips[b] ? p.ow - 1 - x : x;
  int xmin = 0, xcnt = 0;
  int kx[KMAX];
  if (live) {
    double xc, xw;
    taps(ax, xs, xmin, xcnt, xc, xw);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) kx[k] = k < xcnt ? coeff(ax, k, xmin, xc, xw) : 0;
  }
  __syncthreads();
  const int band0 = s_ymin[0];
  const int nband = s_ymin[rows - 1] + s_ycnt[rows - 1] - band0;  // <= kBandMax (host: ksize <= 9)
  if (live) {
    const uint8_t* src = Px<LAYOUT>::at(p.in + srci * p.in_bs, p, band0, xmin);
    const long cs = Px<LAYOUT>::chan_stride(p);
    for (int r = threadIdx.y; r < nband; r += kRowLanes) {
      const uint8_t* row = src + (long)r * p.W * Px<LAYOUT>::kStep;
      int h0 = 1 << (kPrecisionBits - 1), h1 = h0, h2 = h0;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < xcnt) {
          h0 += row[Px<LAYOUT>::kStep * k] * kx[k];
          h1 += row[Px<LAYOUT>::kStep * k + cs] * kx[k];
          h2 += row[Px<LAYOUT>::kStep * k + 2 * cs] * kx[k];
        }
      }
      s_h[r][threadIdx.x] = (uint32_t)clip8(h0) | ((uint32_t)clip8(h1) << 8) | ((uint32_t)clip8(h2) << 16);
    }
  }
  __syncthreads();
  if (!live) return;
  const long plane = (long)p.oh * p.ow;
  float* o = p.out + (long)b * 3 * plane + x;
  for (int r = threadIdx.y; r < rows; r += kRowLanes) {
    const int ymin = s_ymin[r] - band0, ycnt = s_ycnt[r];
    int acc0 = 1 << (kPrecisionBits - 1), acc1 = acc0, acc2 = acc0;
    for (int j = 0; j < ycnt; ++j) {
      const uint32_t hv = s_h[ymin + j][threadIdx.x];
      const int cy = s_ky[r][j];
      acc0 += (int)(hv & 0xffu) * cy;
      acc1 += (int)((hv >> 8) & 0xffu) * cy;
      acc2 += (int)((hv >> 16) & 0xffu) * cy;
    }
    const long off = (long)(y0 + r) * p.ow;
    o[off] = ((float)clip8(acc0) / 255.0f - p.mean[0]) / p.stdv[0];
    o[plane + off] = ((float)clip8(acc1) / 255.0f - p.mean[1]) / p.stdv[1];
    o[2 * plane + off] = ((float)clip8(acc2) / 255.0f - p.mean[2]) / p.stdv[2];
  }
}

// Pillow's kernel size for one axis: ceil(support) * 2 + 1, support = max(in / out, 1)
int axis_ksize(long in, long out) {
  const double scale = (double)in / (double)out;
  const double support = scale < 1.0 ? 1.0 : scale;
  return (int)std::ceil(support) * 2 + 1;
}

// The launch both entries share: the tiled kernel when every axis has at most 9 taps, else the generic one.
template <int LAYOUT>
int launch_preprocess(const PrepArgs& p, hipStream_t stream, const char* what) {
  const int ks = std::max(axis_ksize(p.W, p.ow), axis_ksize(p.H, p.oh));
  if (ks <= 9 && p.B < 65536) {
    const dim3 grid((unsigned)((p.ow + kColsPerBlock - 1) / kColsPerBlock),
                    (unsigned)((p.oh + kRowsPerBlock - 1) / kRowsPerBlock), (unsigned)p.B);
    const dim3 block(kColsPerBlock, kRowLanes);
    if (ks <= 3)
      hipLaunchKernelGGL((preprocess_tiled_kernel<3, LAYOUT>), grid, block, 0, stream, p);
    else if (ks <= 5)
      hipLaunchKernelGGL((preprocess_tiled_kernel<5, LAYOUT>), grid, block, 0, stream, p);
    else
      hipLaunchKernelGGL((preprocess_tiled_kernel<9, LAYOUT>), grid, block, 0, stream, p);
    VIT_LAUNCH_CHECK(what);
  }
  // generic path: any ratio, every weight recomputed per pixel
  const long total = (long)p.B * p.oh * p.ow;
  long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(preprocess_kernel<LAYOUT>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
  VIT_LAUNCH_CHECK(what);
}

PrepArgs make_args(const uint8_t* images, int64_t B, int64_t H, int64_t W, int64_t image_stride, const uint8_t* flips,
                   int64_t out_h, int64_t out_w, const float* mean_std, float* out) {
  PrepArgs p;
  p.in = images;
  p.in_bs = image_stride;
  p.H = (int)H; p.W = (int)W; p.oh = (int)out_h; p.ow = (int)out_w; p.B = (int)B;
  p.flips = flips;
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = mean_std[c];
    p.stdv[c] = mean_std[3 + c];
  }
  p.out = out;
  p.index = nullptr;
  p.n_images = B;
  p.labels_in = nullptr;
  p.labels_out = nullptr;
  return p;
}

// ---------------------------------------------------------------------------------------------------------
// vit_preprocess_u8_ragged: the same transform over decoded image files, whose sizes differ within a batch
// (src/data_loaders.py:100-112 ImageNet, res-vit/data_loaders.py:110-122,191-203: Resize((s, s)) of every image).
// The images lie end to end in one byte array; geom[i] = (offset, H, W) says where image i is. A block owns the
// same 64 x 32 output tile as the tiled kernel, reads its image's row of the table, refuses it when it does not
// fit the array, derives both axes from it and picks its path - uniformly for the block, per image for the launch:
//   <= 9 taps on both axes   the two-pass LDS scheme above with run-time tap counts, specialised for 3 / 5 / 9
//                            (an upscaled, a <= 2x and a <= 4x image: the horizontal weights stay in registers);
//   anything larger          one thread per output pixel. The column's horizontal weights are computed once per
//                            block into the LDS the band does not need here (up to kBandMax taps, a ratio of
//                            66; above that they are recomputed per use - the same expression, the same bits).
// vit_preprocess_u8_ragged_crop adds crops[b] = (top, left, h, w), torchvision's resized_crop (RandomResizedCrop, the
// Inception crop): Pillow's crop(box).resize(size) is this resize run on the sub-rectangle, so the block builds both
// axes - and chooses its path - from the box's (h, w), starts (top * W + left) * 3 bytes into the image and keeps the
// whole image's row pitch 3 * W. A box that is empty or leaves the image is refused like a bad table row. One kernel:
// without crops the box is the image.
struct RaggedArgs {
  const uint8_t* bytes;
  long n_bytes;
  const int64_t* geom;  // [n_images][3] = offset, H, W
  long n_images;
  const int64_t* index;  // [B] or NULL = image b
  long B;
  const uint8_t* flips;
  int oh, ow;
  float mean[3], stdv[3];
  float* out;
  const int64_t* labels_in;
  int64_t* labels_out;
  const int64_t* crops;  // [B][4] = top, left, h, w of output b's crop box, or NULL = the whole image
};

// ceil(support) * 2 + 1 of axis_ksize, on the device
__device__ inline int axis_ksize_dev(const Axis& a) { return (int)ceil(a.support) * 2 + 1; }

// img points at the first pixel the axes address (the image's, or its crop's); row_bytes is the pitch of the whole
// image, which a crop keeps.
template <int KMAX>
__device__ inline void ragged_tiled(const RaggedArgs& p, const uint8_t* img, long row_bytes, const Axis& ax,
                                    const Axis& ay, int b, int y0, int rows, int (*s_ky)[9], int* s_ymin, int* s_ycnt,
                                    uint32_t (*s_h)[kColsPerBlock]) {
#pragma clang fp contract(off)
  const int tid = threadIdx.y * kColsPerBlock + threadIdx.x;
  if (tid < rows) {
    int ymin, ycnt;
    double yc, yw;
    taps(ay, y0 + tid, ymin, ycnt, yc, yw);
    s_ymin[tid] = ymin;
    s_ycnt[tid] = ycnt;
    for (int j = 0; j < KMAX; ++j) s_ky[tid][j] = j < ycnt ? coeff(ay, j, ymin, yc, yw) : 0;
  }
  const int x = blockIdx.x * kColsPerBlock + threadIdx.x;
  const bool live = x < p.ow;
  const int xs = live && p.flips && p.flips[b] ? p.ow - 1 - x : x;
  int xmin = 0, xcnt = 0;
  int kx[KMAX];
  if (live) {
    double xc, xw;
    taps(ax, xs, xmin, xcnt, xc, xw);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) kx[k] = k < xcnt ? coeff(ax, k, xmin, xc, xw) : 0;
  }
  __syncthreads();
  const int band0 = s_ymin[0];
  const int nband = s_ymin[rows - 1] + s_ycnt[rows - 1] - band0;  // <= kBandMax: both axes have <= 9 taps
  if (live) {
    const uint8_t* src = img + (long)band0 * row_bytes + (long)xmin * 3;
    for (int r = threadIdx.y; r < nband; r += kRowLanes) {
      const uint8_t* row = src + (long)r * row_bytes;
      int h0 = 1 << (kPrecisionBits - 1), h1 = h0, h2 = h0;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < xcnt) {
          h0 += row[3 * k] * kx[k];
          h1 += row[3 * k + 1] * kx[k];
          h2 += row[3 * k + 2] * kx[k];
        }
      }
      s_h[r][threadIdx.x] = (uint32_t)clip8(h0) | ((uint32_t)clip8(h1) << 8) | ((uint32_t)clip8(h2) << 16);
    }
  }
  __syncthreads();
  if (!live) return;
  const long plane = (long)p.oh * p.ow;
  float* o = p.out + (long)b * 3 * plane + x;
  for (int r = threadIdx.y; r < rows; r += kRowLanes) {
    const int ymin = s_ymin[r] - band0, ycnt = s_ycnt[r];
    int acc0 = 1 << (kPrecisionBits - 1), acc1 = acc0, acc2 = acc0;
    for (int j = 0; j < ycnt; ++j) {
      const uint32_t hv = s_h[ymin + j][threadIdx.x];
      const int cy = s_ky[r][j];
      acc0 += (int)(hv & 0xffu) * cy;
      acc1 += (int)((hv >> 8) & 0xffu) * cy;
      acc2 += (int)((hv >> 16) & 0xffu) * cy;
    }
    const long off = (long)(y0 + r) * p.ow;
    o[off] = ((float)clip8(acc0) / 255.0f - p.mean[0]) / p.stdv[0];
    o[plane + off] = ((float)clip8(acc1) / 255.0f - p.mean[1]) / p.stdv[1];
    o[2 * plane + off] = ((float)clip8(acc2) / 255.0f - p.mean[2]) / p.stdv[2];
  }
}

// the per-pixel body for a block whose image has more than 9 taps on an axis; ksx = the horizontal kernel size
__device__ inline void ragged_pixel(const RaggedArgs& p, const uint8_t* img, long row_bytes, const Axis& ax,
                                    const Axis& ay, int ksx, int b, int y0, int rows,
                                    uint32_t (*s_h)[kColsPerBlock]) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * kColsPerBlock + threadIdx.x;
  const bool live = x < p.ow;
  const int xs = live && p.flips && p.flips[b] ? p.ow - 1 - x : x;
  int xmin = 0, xcnt = 0;
  double xc = 0.0, xw = 0.0;
  if (live) taps(ax, xs, xmin, xcnt, xc, xw);
  const bool held = ksx <= kBandMax;  // xcnt <= ksx: column threadIdx.x's weights fit s_h[.][threadIdx.x]
  if (held) {
    for (int k = threadIdx.y; k < xcnt; k += kRowLanes) s_h[k][threadIdx.x] = (uint32_t)coeff(ax, k, xmin, xc, xw);
    __syncthreads();
  }
  if (!live) return;
  const long plane = (long)p.oh * p.ow;
  float* o = p.out + (long)b * 3 * plane + x;
  for (int r = threadIdx.y; r < rows; r += kRowLanes) {
    int ymin, ycnt;
    double yc, yw;
    taps(ay, y0 + r, ymin, ycnt, yc, yw);
    int acc0 = 1 << (kPrecisionBits - 1), acc1 = acc0, acc2 = acc0;
    for (int j = 0; j < ycnt; ++j) {
      const uint8_t* row = img + (long)(ymin + j) * row_bytes + (long)xmin * 3;
      int h0 = 1 << (kPrecisionBits - 1), h1 = h0, h2 = h0;
      for (int k = 0; k < xcnt; ++k) {
        const int c = held ? (int)s_h[k][threadIdx.x] : coeff(ax, k, xmin, xc, xw);
        h0 += row[3 * k] * c;
        h1 += row[3 * k + 1] * c;
        h2 += row[3 * k + 2] * c;
      }
      const int cy = coeff(ay, j, ymin, yc, yw);
      acc0 += clip8(h0) * cy;
      acc1 += clip8(h1) * cy;
      acc2 += clip8(h2) * cy;
    }
    const long off = (long)(y0 + r) * p.ow;
    o[off] = ((float)clip8(acc0) / 255.0f - p.mean[0]) / p.stdv[0];
    o[plane + off] = ((float)clip8(acc1) / 255.0f - p.mean[1]) / p.stdv[1];
    o[2 * plane + off] = ((float)clip8(acc2) / 255.0f - p.mean[2]) / p.stdv[2];
  }
}

__global__ void __launch_bounds__(kColsPerBlock* kRowLanes) preprocess_ragged_kernel(RaggedArgs p) {
  __shared__ int s_ky[kRowsPerBlock][9];
  __shared__ int s_ymin[kRowsPerBlock], s_ycnt[kRowsPerBlock];
  __shared__ uint32_t s_h[kBandMax][kColsPerBlock];  // 34 KB: the band, or the per-pixel path's column weights
  const int y0 = blockIdx.y * kRowsPerBlock;
  const int rows = p.oh - y0 < kRowsPerBlock ? p.oh - y0 : kRowsPerBlock;
  // grid.z covers the batch, strided where the batch is larger than a grid may be
  for (long bl = blockIdx.z; bl < p.B; bl += gridDim.z) {
    const int b = (int)bl;
    // this block's image, or none: everything below is uniform over the block
    long srci = p.index ? p.index[b] : bl;
    long off = 0, H = 0, W = 0;
    bool ok = srci >= 0 && srci < p.n_images;
    if (ok) {
      off = p.geom[srci * 3];
      H = p.geom[srci * 3 + 1];
      W = p.geom[srci * 3 + 2];
      // H, W < 2^15, so 3 * H * W < 2^32 and the comparison cannot overflow
      ok = H > 0 && H < (1 << 15) && W > 0 && W < (1 << 15) && off >= 0 && 3 * H * W <= p.n_bytes &&
           off <= p.n_bytes - 3 * H * W;
    }
    // the crop box of this output (torchvision's resized_crop): the resize below runs on the sub-rectangle
    long top = 0, left = 0, ch = H, cw = W;
    if (ok && p.crops) {
      top = p.crops[bl * 4];
      left = p.crops[bl * 4 + 1];
      ch = p.crops[bl * 4 + 2];
      cw = p.crops[bl * 4 + 3];
      // each bound is checked against H, W < 2^15 before it enters a sum, so nothing overflows
      ok = ch > 0 && cw > 0 && top >= 0 && left >= 0 && ch <= H && cw <= W && top <= H - ch && left <= W - cw;
    }
    if (threadIdx.x == 0 && threadIdx.y == 0 && blockIdx.x == 0 && blockIdx.y == 0 && p.labels_in && p.labels_out)
      p.labels_out[b] = ok ? p.labels_in[srci] : -1;
    if (!ok) {  // never read through: NaN for this output alone
      const int xo = blockIdx.x * kColsPerBlock + threadIdx.x;
      if (xo < p.ow) {
        const long pl = (long)p.oh * p.ow;
        float* o = p.out + (long)b * 3 * pl + xo;
        for (int r = threadIdx.y; r < rows; r += kRowLanes)
          for (int c = 0; c < 3; ++c) o[c * pl + (long)(y0 + r) * p.ow] = __builtin_nanf("");
      }
      continue;
    }
    const Axis ax = make_axis((int)cw, p.ow), ay = make_axis((int)ch, p.oh);
    const int ksx = axis_ksize_dev(ax), ksy = axis_ksize_dev(ay);
    const int ks = ksx > ksy ? ksx : ksy;
    const long row_bytes = W * 3;  // the whole image's pitch, also under a crop
    const uint8_t* img = p.bytes + off + (top * W + left) * 3;
    if (ks <= 3)
      ragged_tiled<3>(p, img, row_bytes, ax, ay, b, y0, rows, s_ky, s_ymin, s_ycnt, s_h);
    else if (ks <= 5)
      ragged_tiled<5>(p, img, row_bytes, ax, ay, b, y0, rows, s_ky, s_ymin, s_ycnt, s_h);
    else if (ks <= 9)
      ragged_tiled<9>(p, img, row_bytes, ax, ay, b, y0, rows, s_ky, s_ymin, s_ycnt, s_h);
    else
      ragged_pixel(p, img, row_bytes, ax, ay, ksx, b, y0, rows, s_h);
    __syncthreads();  // the next image of this block reuses the LDS
  }
}

}  // namespace

namespace {
// the one launch behind vit_preprocess_u8_ragged (crops == NULL) and vit_preprocess_u8_ragged_crop
int launch_ragged(const char* what, const uint8_t* bytes, int64_t n_bytes, const int64_t* geom, int64_t n_images,
                  const int64_t* index, int64_t B, const uint8_t* flips, const int64_t* crops, int64_t out_h,
                  int64_t out_w, const float* mean_std, float* out, const int64_t* labels_in, int64_t* labels_out,
                  vit_stream_t stream) {
  VIT_CHECK_ARG(bytes && geom && out && mean_std, "%s: null bytes / geom / out / mean_std", what);
  VIT_CHECK_ARG(B > 0 && n_images > 0 && n_bytes > 0 && out_h > 0 && out_w > 0,
                "%s: B, n_images, n_bytes and the output size must be positive", what);
  VIT_CHECK_ARG(out_h < (1 << 15) && out_w < (1 << 15) && B < (1LL << 31) && B * out_h * out_w < (1LL << 40) &&
                    n_images < (1LL << 40),
                "%s: sizes too large", what);
  RaggedArgs p;
  p.bytes = bytes;
  p.n_bytes = n_bytes;
  p.geom = geom;
  p.n_images = n_images;
  p.index = index;
  p.B = B;
  p.flips = flips;
  p.oh = (int)out_h;
  p.ow = (int)out_w;
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = mean_std[c];
    p.stdv[c] = mean_std[3 + c];
  }
  p.out = out;
  p.labels_in = labels_in;
  p.labels_out = labels_out;
  p.crops = crops;
  const long cb = (out_w + kColsPerBlock - 1) / kColsPerBlock, rb = (out_h + kRowsPerBlock - 1) / kRowsPerBlock;
  // at most 65535 in z and fewer than 2^32 threads in the grid: the kernel strides the batch over z
  const long z = std::max(1L, std::min({(long)B, 65535L, ((1L << 24) - 1) / (cb * rb)}));
  hipLaunchKernelGGL(preprocess_ragged_kernel, dim3((unsigned)cb, (unsigned)rb, (unsigned)z),
                     dim3(kColsPerBlock, kRowLanes), 0, (hipStream_t)stream, p);
  VIT_LAUNCH_CHECK(what);
}
}  // namespace

extern "C" int vit_preprocess_u8_ragged(const uint8_t* bytes, int64_t n_bytes, const int64_t* geom, int64_t n_images,
                                        const int64_t* index, int64_t B, const uint8_t* flips, int64_t out_h,
                                        int64_t out_w, const float* mean_std, float* out, const int64_t* labels_in,
                                        int64_t* labels_out, vit_stream_t stream) {
  return launch_ragged("vit_preprocess_u8_ragged", bytes, n_bytes, geom, n_images, index, B, flips, nullptr, out_h,
                       out_w, mean_std, out, labels_in, labels_out, stream);
}

extern "C" int vit_preprocess_u8_ragged_crop(const uint8_t* bytes, int64_t n_bytes, const int64_t* geom,
                                             int64_t n_images, const int64_t* index, int64_t B, const uint8_t* flips,
                                             const int64_t* crops, int64_t out_h, int64_t out_w,
                                             const float* mean_std, float* out, const int64_t* labels_in,
                                             int64_t* labels_out, vit_stream_t stream) {
  return launch_ragged("vit_preprocess_u8_ragged_crop", bytes, n_bytes, geom, n_images, index, B, flips, crops, out_h,
                       out_w, mean_std, out, labels_in, labels_out, stream);
}

extern "C" int vit_preprocess_u8(const uint8_t* images, int64_t B, int64_t H, int64_t W, int64_t image_stride,
                                 const uint8_t* flips, int64_t out_h, int64_t out_w, const float* mean_std,
                                 float* out, vit_stream_t stream) {
  VIT_CHECK_ARG(images && out && mean_std && B > 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0,
                "vit_preprocess_u8: bad args");
  VIT_CHECK_ARG(image_stride >= H * W * 3, "vit_preprocess_u8: image_stride %lld < H*W*3", (long long)image_stride);
  VIT_CHECK_ARG(H < (1 << 15) && W < (1 << 15) && out_h < (1 << 15) && out_w < (1 << 15) &&
                    B * out_h * out_w < (1LL << 40),
                "vit_preprocess_u8: sizes too large");
  const PrepArgs p = make_args(images, B, H, W, image_stride, flips, out_h, out_w, mean_std, out);
  return launch_preprocess<kLayoutHWC>(p, (hipStream_t)stream, "vit_preprocess_u8");
}

extern "C" int vit_preprocess_u8_gather(const uint8_t* images, int64_t n_images, int32_t layout, int64_t H, int64_t W,
                                        int64_t image_stride, const int64_t* index, int64_t B, const uint8_t* flips,
                                        int64_t out_h, int64_t out_w, const float* mean_std, float* out,
                                        const int64_t* labels_in, int64_t* labels_out, vit_stream_t stream) {
  VIT_CHECK_ARG(images && index && out && mean_std, "vit_preprocess_u8_gather: null images / index / out / mean_std");
  VIT_CHECK_ARG(B > 0 && n_images > 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0,
                "vit_preprocess_u8_gather: B, n_images and every size must be positive");
  VIT_CHECK_ARG(layout == kLayoutHWC || layout == kLayoutCHW, "vit_preprocess_u8_gather: layout %d (0 = HWC, 1 = CHW)",
                (int)layout);
  VIT_CHECK_ARG(H < (1 << 15) && W < (1 << 15) && out_h < (1 << 15) && out_w < (1 << 15) && B < (1LL << 31) &&
                    B * out_h * out_w < (1LL << 40) && n_images < (1LL << 40),
                "vit_preprocess_u8_gather: sizes too large");
  VIT_CHECK_ARG(image_stride >= H * W * 3 && image_stride < (1LL << 40),
                "vit_preprocess_u8_gather: image_stride %lld < H*W*3", (long long)image_stride);
  PrepArgs p = make_args(images, B, H, W, image_stride, flips, out_h, out_w, mean_std, out);
  p.index = index;
  p.n_images = n_images;
  p.labels_in = labels_in;
  p.labels_out = labels_out;
  if (layout == kLayoutCHW) return launch_preprocess<kLayoutCHW>(p, (hipStream_t)stream, "vit_preprocess_u8_gather");
  return launch_preprocess<kLayoutHWC>(p, (hipStream_t)stream, "vit_preprocess_u8_gather");
}
