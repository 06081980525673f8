// Batch mixing for from-scratch training: Mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019) in timm's batch mode,
// as one HBM-bound pass over the f32 NCHW batch the input transform produced: two reads and one write per element.
//   inside sample b's box      out = x[pair[b]]                                   (an exact copy: CutMix's patch)
//   elsewhere                  out = lam[b] x[b] + (1 - lam[b]) x[pair[b]]        (Mixup; lam = 1 leaves x[b] as it is)
// The policy (which partner, which lam, which box) is the host's (vitmi.augment.BatchMixer); the kernel takes it as
// three small device arrays, so one launch serves Mixup, CutMix, and a batch left alone.
#include "common.h"

namespace {

struct MixArgs {
  const float* x;
  float* out;
  long B, plane3;  // samples; 3 * H * W
  int H, W;
  const int64_t* pair;  // [B]
  const float* lam;     // [B]
  const int64_t* box;   // [B][4] = y0, y1, x0, x1, half-open
};

// lam a + (1 - lam) b within 2^-24 (|lam a| + 2 |(1 - lam) b|): 1 - lam = om + eo exactly (om the rounded difference,
// eo its error, both f32), so the partner's term is rounded once, by the inner fma, and the sum once, by the outer.
// A weight of exactly 1 or 0 passes its operand through untouched (a batch left alone is a copy, whatever the
// partner holds).
struct Blend {
  float lam, om, eo;
  __device__ explicit Blend(float l) : lam(l) {
#pragma clang fp contract(off)
    om = 1.0f - l;
    eo = (1.0f - om) - l;
  }
  __device__ inline float operator()(float a, float b) const {
    if (lam == 1.0f) return a;
    if (lam == 0.0f) return b;
    return fmaf(lam, a, fmaf(om, b, eo * b));
  }
};

// VEC = 4: W % 4 == 0 and 16-B aligned pointers, so four neighbours of one image row move as one float4; the box
// edge may fall inside the four and is decided per element. VEC = 1: any W, any alignment.
template <int VEC>
__global__ void __launch_bounds__(256) mix_batch_kernel(MixArgs p) {
  const long plane = (long)p.H * p.W;
  const long total = p.B * p.plane3 / VEC;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long e = i * VEC;
    const long b = e / p.plane3;
    const long rem = e - b * p.plane3;
    const int pix = (int)(rem % plane);
    const int y = pix / p.W, x0 = pix - y * p.W;
    const int64_t pr = p.pair[b];
    if (pr < 0 || pr >= p.B) {  // never read through: this sample alone is NaN
      const float nan = __builtin_nanf("");
      if (VEC == 4)
        *reinterpret_cast<float4*>(p.out + e) = make_float4(nan, nan, nan, nan);
      else
        p.out[e] = nan;
      continue;
    }
    const Blend blend(p.lam[b]);
    const int64_t* bx = p.box + b * 4;
    const bool in_rows = y >= bx[0] && y < bx[1];
    const int64_t bx0 = bx[2], bx1 = bx[3];
    const long pe = pr * p.plane3 + rem;
    if (VEC == 4) {
      const float4 a = *reinterpret_cast<const float4*>(p.x + e);
      const float4 q = *reinterpret_cast<const float4*>(p.x + pe);
      float4 o;
      o.x = in_rows && x0 >= bx0 && x0 < bx1 ? q.x : blend(a.x, q.x);
      o.y = in_rows && x0 + 1 >= bx0 && x0 + 1 < bx1 ? q.y : blend(a.y, q.y);
      o.z = in_rows && x0 + 2 >= bx0 && x0 + 2 < bx1 ? q.z : blend(a.z, q.z);
      o.w = in_rows && x0 + 3 >= bx0 && x0 + 3 < bx1 ? q.w : blend(a.w, q.w);
      *reinterpret_cast<float4*>(p.out + e) = o;
    } else {
      const float a = p.x[e], q = p.x[pe];
      p.out[e] = in_rows && x0 >= bx0 && x0 < bx1 ? q : blend(a, q);
    }
  }
}

}  // namespace

extern "C" int vit_mix_batch(const float* x, float* out, int64_t B, int64_t H, int64_t W, const int64_t* pair,
                             const float* lam, const int64_t* box, vit_stream_t stream) {
  VIT_CHECK_ARG(x && out && pair && lam && box, "vit_mix_batch: null x / out / pair / lam / box");
  VIT_CHECK_ARG(B > 0 && H > 0 && W > 0, "vit_mix_batch: B, H and W must be positive");
  VIT_CHECK_ARG(H < (1 << 15) && W < (1 << 15) && B < (1LL << 31) && B * 3 * H * W < (1LL << 40),
                "vit_mix_batch: sizes too large");
  const int64_t n = B * 3 * H * W;
  VIT_CHECK_ARG((uintptr_t)out + (uintptr_t)n * 4 <= (uintptr_t)x || (uintptr_t)x + (uintptr_t)n * 4 <= (uintptr_t)out,
                "vit_mix_batch: out must not overlap x");
  MixArgs p;
  p.x = x;
  p.out = out;
  p.B = B;
  p.plane3 = 3 * H * W;
  p.H = (int)H;
  p.W = (int)W;
  p.pair = pair;
  p.lam = lam;
  p.box = box;
  const bool vec = W % 4 == 0 && ((uintptr_t)x | (uintptr_t)out) % 16 == 0;
  const long work = vec ? n / 4 : n;
  long blocks = (work + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  if (vec)
    hipLaunchKernelGGL(mix_batch_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(mix_batch_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  VIT_LAUNCH_CHECK("vit_mix_batch");
}
