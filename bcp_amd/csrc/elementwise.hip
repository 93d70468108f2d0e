// bcp_amd/csrc/elementwise.hip -- HBM-bound BCP ops for gfx950: box copy-paste mix (A3+A4),
// pseudo-label (A5), EMA (A10), SGD/Adam (A11), label casts, weight packing.
// Every kernel is a 16-B-per-lane vectorised grid-stride stream (guide Appendix B "element-wise").
#include "common.h"
#include "../../include/bcp_hip.h"

// EMA / SGD must round every product and sum separately (bit-exact vs the reference's mul_/add_ chain):
// hipcc defaults to -ffp-contract=fast, which would fuse __fmul_rn + __fadd_rn into v_fma_f32.
#pragma clang fp contract(off)
namespace bcp {
__device__ __forceinline__ float rn_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float rn_add(float a, float b) { return a + b; }
}  // namespace bcp

namespace bcp {

constexpr int kMaskBoxesMax = 32;  // bcp_mask_boxes: boxes per launch (the reference needs 27)

static inline int stream_grid(long long n_items, int block) {
  long long g = (n_items + block - 1) / block;
  if (g > 2048) g = 2048;  // 256 CUs x 8 blocks, grid-stride the rest (guide G11)
  if (g < 1) g = 1;
  return (int)g;
}

// ---------------------------------------------------------------- mix (A3+A4)
// out = a outside the box, b inside (reference: a*mask + b*(1-mask), mask = 1 outside the box;
// LA_BCP_train.py:248-251, ACDC_BCP_train.py:372-373, utils/BCP_utils.py:18-28).
// Layout [N][D][H][W][C] with C*W % 4 == 0; the box is in (d,h,w) voxel coordinates.
template <int U>
__global__ __launch_bounds__(256) void k_mix_box(const float* __restrict__ a, const float* __restrict__ b,
                                                 float* __restrict__ out, long long n_vec, int D, int H, int W, int C,
                                                 int d0, int d1, int h0, int h1, int w0, int w1) {
  // (round 3: 32-bit index arithmetic -- the first version spent three 64-bit divisions per 16 bytes -- and U independent
  //  vectors per thread; the launcher guarantees n_vec < 2^29.  Round 4: U = 1 for launches under 4 M floats -- one LA volume with
  //  U = 4 is 245 workgroups, less than one per CU, and the launch is latency: 31 us alone for 12 MB)
  const unsigned nv = (unsigned)n_vec, stride = gridDim.x * blockDim.x;
  const unsigned rowlen = (unsigned)(W * C);  // floats per (n,d,h) row
  for (unsigned i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < nv; i0 += U * stride) {
    float4 va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned i = i0 + u * stride;
      if (i < nv) { va[u] = ld4(a + (size_t)i * 4); vb[u] = ld4(b + (size_t)i * 4); }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned i = i0 + u * stride;
      if (i >= nv) continue;
      const unsigned e = i * 4u;
      const unsigned row = e / rowlen, inrow = e - row * rowlen;
      const int h = (int)(row % (unsigned)H), d = (int)((row / (unsigned)H) % (unsigned)D);
      const bool dh_in = (d >= d0) & (d < d1) & (h >= h0) & (h < h1);
      float4 vo;
      float* po = &vo.x;
      const float* pa = &va[u].x;
      const float* pb = &vb[u].x;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int w = (int)((inrow + k) / (unsigned)C);
        const bool in = dh_in & (w >= w0) & (w < w1);
        po[k] = in ? pb[k] : pa[k];
      }
      st4(out + (size_t)i * 4, vo);
    }
  }
}

// Single-channel images (C == 1, W % 4 == 0: every input of the three training loops), round 5.  The general kernel above spends six
// 32-bit divisions per 16 bytes on its (d, h, w) coordinates and reads both inputs everywhere; here a workgroup row (blockIdx.y) is one
// (n, d) slice, the row index inside it is one multiply-high by a host-computed reciprocal, and `b` is read only where the box is:
// algorithmic bytes 8 (a) + 8 (out) + 8 x box fraction per voxel -- 5.0 us for one 8 MB LA batch, 3.6 TB/s (profiles/r05_t2_pmc_ops.txt).
// (The "30 us, 58.5 MB written" rounds 2-4 reported for the mix were the profiling script's own torch.randn launches, DESIGN.md section 5;
// inside the step the two kernels are indistinguishable: 5.541 vs 5.524 ms.)
__global__ __launch_bounds__(256) void k_mix_box_c1(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                                    int HW4 /* float4 per slice */, int W4 /* float4 per image row */,
                                                    unsigned magic /* ceil(2^32 / W4) */, int D, int d0, int d1, int h0, int h1, int w0,
                                                    int w1) {
  const int slice = blockIdx.y;                     // n * D + d
  const int d = slice % D;
  const bool d_in = (d >= d0) & (d < d1);           // workgroup-uniform
  const long long base = (long long)slice * HW4;
  for (int s = blockIdx.x * 256 + threadIdx.x; s < HW4; s += gridDim.x * 256) {
    float4 v = ld4(a + (base + s) * 4);
    if (d_in) {
      const int h = (int)__umulhi((unsigned)s, magic);          // s / W4 (exact: the launcher checks HW4 * W4 < 2^32)
      const int w = (s - h * W4) * 4;
      if ((h >= h0) & (h < h1) & (w + 3 >= w0) & (w < w1)) {
        const float4 vb = ld4(b + (base + s) * 4);
        if ((w >= w0) & (w < w1)) v.x = vb.x;
        if ((w + 1 >= w0) & (w + 1 < w1)) v.y = vb.y;
        if ((w + 2 >= w0) & (w + 2 < w1)) v.z = vb.z;
        if ((w + 3 >= w0) & (w + 3 < w1)) v.w = vb.w;
      }
    }
    st4(out + (base + s) * 4, v);
  }
}

// ---------------------------------------------------------------- region masks (union of boxes)
// The reference's other copy-paste regions -- 27 small boxes (utils/BCP_utils.py:30-46 random_mask), 9 boxes (ACDC_BCP_train.py:142-154
// random_mask), one slab / band (utils/BCP_utils.py:48-56 concate_mask, ACDC_BCP_train.py:156-164 contact_mask) -- as ONE uint8 map
// [N][D][H][W], 0 inside the union and 1 elsewhere (the loss kernels' mask_or_null: 1 = image term).  The boxes travel by value.
struct MaskBoxes {
  int k;
  int b[kMaskBoxesMax][6];  // d0, d1, h0, h1, w0, w1 (half-open, clamped to the volume by the launcher)
};

// one mask nibble (bit j = voxel j is inside the union) -> four mask bytes
__device__ __forceinline__ unsigned mask_word(unsigned nib, unsigned flip) {
  const unsigned in = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
  return (in ^ flip) & 0x01010101u;
}

// Shaped like k_mix_box_c1: a workgroup row (blockIdx.y) is one (n, d) slice, so "does this box contain d" is workgroup-uniform and the
// boxes that do not are skipped before any per-thread work.  A thread owns 16 voxels along W: it collects a 16-bit "inside" set over the
// boxes and writes the 16 bytes with one vector store (V16), or as up to four 4-byte words where W % 16 != 0 (rows are then only 4-B aligned).
template <bool V16>
__global__ __launch_bounds__(256) void k_mask_boxes(uint8_t* __restrict__ out, int D, int H, int W, int W16 /* ceil(W / 16) */,
                                                    MaskBoxes bx, unsigned flip /* 0x01010101: 1 outside; 0: complement */) {
  const int slice = blockIdx.y;  // n * D + d
  const int d = slice % D;
  const long long base = (long long)slice * H * W;
  const int items = H * W16;
  for (int s = blockIdx.x * 256 + threadIdx.x; s < items; s += gridDim.x * 256) {
    const int h = s / W16, w = (s - h * W16) * 16;
    unsigned in = 0;
    // chunks of eight boxes with compile-time indices: the boxes are kernel arguments, so each chunk arrives as a few wide scalar loads
    // issued together, where a loop over a run-time index would wait for one scalar load per box (what of this is
    // measured).  Slots past bx.k hold empty boxes (d0 == d1 == 0) and fail the first test.
#pragma unroll
    for (int k0 = 0; k0 < kMaskBoxesMax; k0 += 8) {
      if (k0 >= bx.k) break;  // workgroup-uniform
#pragma unroll
      for (int k = k0; k < k0 + 8; ++k) {
        if ((d < bx.b[k][0]) | (d >= bx.b[k][1])) continue;  // workgroup-uniform
        if ((h < bx.b[k][2]) | (h >= bx.b[k][3])) continue;
        int lo = bx.b[k][4] - w, hi = bx.b[k][5] - w;
        lo = lo < 0 ? 0 : lo;
        hi = hi > 16 ? 16 : hi;
        if (lo < hi) in |= ((1u << hi) - 1u) & ~((1u << lo) - 1u);
      }
    }
    uint8_t* p = out + base + (long long)h * W + w;
    if (V16) {
      uint4 v;
      v.x = mask_word(in, flip);
      v.y = mask_word(in >> 4, flip);
      v.z = mask_word(in >> 8, flip);
      v.w = mask_word(in >> 12, flip);
      *reinterpret_cast<uint4*>(p) = v;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (w + 4 * j < W) *reinterpret_cast<unsigned*>(p + 4 * j) = mask_word(in >> (4 * j), flip);  // W % 4 == 0: whole words only
    }
  }
}

// out = mask ? a : b per voxel, a select (values pass through bit for bit, NaN and -0.0 included -- as k_mix_box_c1 does).  blockIdx.y is
// the sample; four mask bytes arrive as one 32-bit word per float4 and `b` is read only where one of them is zero: 4 (a) + 4 (out) + 1 (mask)
// + 4 x zero fraction bytes per voxel.
__global__ __launch_bounds__(256) void k_mix_mask(const float* __restrict__ a, const float* __restrict__ b, const uint8_t* __restrict__ mask,
                                                  float* __restrict__ out, int V4 /* float4 per sample */, long long mask_sample_stride) {
  const long long base = (long long)blockIdx.y * V4;
  const unsigned* __restrict__ m = reinterpret_cast<const unsigned*>(mask + (long long)blockIdx.y * mask_sample_stride);
  for (int s = blockIdx.x * 256 + threadIdx.x; s < V4; s += gridDim.x * 256) {
    const unsigned mw = m[s];
    float4 v = ld4(a + (base + s) * 4);
    if ((mw - 0x01010101u) & ~mw & 0x80808080u) {  // some byte is zero
      const float4 vb = ld4(b + (base + s) * 4);
      if (!(mw & 0x000000ffu)) v.x = vb.x;
      if (!(mw & 0x0000ff00u)) v.y = vb.y;
      if (!(mw & 0x00ff0000u)) v.z = vb.z;
      if (!(mw & 0xff000000u)) v.w = vb.w;
    }
    st4(out + (base + s) * 4, v);
  }
}

// ---------------------------------------------------------------- pseudo-label (A5)
// LA / pancreas: softmax over 2 channels, (p1 >= thres) -> uint8 (LA_BCP_train.py:57-60).
__global__ __launch_bounds__(256) void k_plabel_bin(const float* __restrict__ logits, uint8_t* __restrict__ out,
                                                    long long n_vec, float thres) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += stride) {
    const float4 l0 = ld4(logits + i * 8), l1 = ld4(logits + i * 8 + 4);
    const float x[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
    uchar4 r;
    unsigned char* pr = &r.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) pr[k] = plabel_bin_of(x[2 * k], x[2 * k + 1], thres);
    *reinterpret_cast<uchar4*>(out + i * 4) = r;
  }
}

// ACDC: softmax over 4 channels then argmax, first maximum wins (ACDC_BCP_train.py:112-114).
__global__ __launch_bounds__(256) void k_plabel_argmax4(const float* __restrict__ logits, uint8_t* __restrict__ out,
                                                        long long n_pix) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += stride) {
    const float4 l = ld4(logits + i * 4);
    out[i] = plabel_argmax4_of(l.x, l.y, l.z, l.w);
  }
}

// ---------------------------------------------------------------- EMA (A10)
// dst = alpha*dst + (1-alpha)*src with the reference's two roundings per term
// (ema.mul_(alpha).add_((1-alpha)*param), utils/BCP_utils.py:78-81); no FMA contraction.
__global__ __launch_bounds__(256) void k_ema(float* __restrict__ dst, const float* __restrict__ src, long long n,
                                             float alpha, float one_minus_alpha) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long nv = n / 4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    float4 d = ld4(dst + i * 4);
    const float4 s = ld4(src + i * 4);
    d.x = rn_add(rn_mul(d.x, alpha), rn_mul(one_minus_alpha, s.x));
    d.y = rn_add(rn_mul(d.y, alpha), rn_mul(one_minus_alpha, s.y));
    d.z = rn_add(rn_mul(d.z, alpha), rn_mul(one_minus_alpha, s.z));
    d.w = rn_add(rn_mul(d.w, alpha), rn_mul(one_minus_alpha, s.w));
    st4(dst + i * 4, d);
  }
  for (long long i = nv * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    dst[i] = rn_add(rn_mul(dst[i], alpha), rn_mul(one_minus_alpha, src[i]));
}

// ---------------------------------------------------------------- SGD / Adam (A11)
// torch.optim.SGD (LA_BCP_train.py:218): g += wd*p; buf = m*buf + g (first step: buf = g); p -= lr*buf.
// Optional fused EMA of a teacher copy (28 B/param instead of 20 + 12).
__global__ __launch_bounds__(256) void k_sgd(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                             float* __restrict__ ema, long long n, float lr, float momentum, float wd,
                                             float gscale, int first_step, float alpha, float one_minus_alpha) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float pv = p[i];
    const float gv = rn_add(g[i] * gscale, rn_mul(wd, pv));
    const float bv = first_step ? gv : rn_add(rn_mul(momentum, buf[i]), gv);
    buf[i] = bv;
    pv = rn_add(pv, rn_mul(-lr, bv));
    p[i] = pv;
    if (ema) ema[i] = rn_add(rn_mul(ema[i], alpha), rn_mul(one_minus_alpha, pv));
  }
}

// torch.optim.Adam defaults (pancreas/dataloaders.py:182): bias-corrected, eps outside the sqrt.
__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, long long n, float lr, float b1, float b2, float eps,
                                              float bc1, float bc2_sqrt, float gscale) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gv = g[i] * gscale;
    const float mv = m[i] * b1 + (1.f - b1) * gv;
    const float vv = v[i] * b2 + (1.f - b2) * gv * gv;
    m[i] = mv;
    v[i] = vv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    p[i] = p[i] - (lr / bc1) * (mv / denom);
  }
}

// ---------------------------------------------------------------- casts / fills
__global__ __launch_bounds__(256) void k_i64_to_u8(const long long* __restrict__ in, uint8_t* __restrict__ out, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (uint8_t)in[i];
}
__global__ __launch_bounds__(256) void k_f32_to_u8(const float* __restrict__ in, uint8_t* __restrict__ out, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (uint8_t)in[i];
}
__global__ __launch_bounds__(256) void k_u8_to_f32(const uint8_t* __restrict__ in, float* __restrict__ out, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (float)in[i];
}
__global__ __launch_bounds__(256) void k_u8_to_i64(const uint8_t* __restrict__ in, long long* __restrict__ out, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (long long)in[i];
}
__global__ __launch_bounds__(256) void k_axpy(float* __restrict__ y, const float* __restrict__ x, long long n, float a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = y[i] + a * x[i];
}

// Counter-hash Bernoulli keep-masks for throughput runs (parity runs inject masks instead).
// seed_dev != nullptr: the seed lives in device memory (a launch captured in a HIP graph keeps its arguments; the seed still changes
// every pass -- bcp_store_u64 writes it ahead of the graph launch)
__global__ __launch_bounds__(256) void k_bernoulli_f32(float* __restrict__ out, long long n, float p_keep, float keep_value,
                                                       unsigned seed_lo, unsigned seed_hi, const unsigned long long* __restrict__ seed_dev) {
  if (seed_dev) { const unsigned long long s = *seed_dev; seed_lo = (unsigned)s; seed_hi = (unsigned)(s >> 32); }
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    out[i] = bern_keep(i, seed_lo, seed_hi, p_keep) ? keep_value : 0.f;
  }
}
__global__ __launch_bounds__(256) void k_bernoulli_u8(uint8_t* __restrict__ out, long long n, float p_keep,
                                                      unsigned seed_lo, unsigned seed_hi, const unsigned long long* __restrict__ seed_dev) {
  if (seed_dev) { const unsigned long long s = *seed_dev; seed_lo = (unsigned)s; seed_hi = (unsigned)(s >> 32); }
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    out[i] = bern_keep(i, seed_lo, seed_hi, p_keep) ? 1 : 0;
  }
}

}  // namespace bcp

using namespace bcp;

extern "C" int bcp_mix_box(const float* a, const float* b, float* out, int N, int D, int H, int W, int C,
                           const int* box6, void* stream) {
  BCP_REQUIRE(a && b && out && box6, "bcp_mix_box: null pointer");
  BCP_REQUIRE(aligned16(a) && aligned16(b) && aligned16(out), "bcp_mix_box: pointers must be 16-B aligned");
  BCP_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && C > 0, "bcp_mix_box: bad extents");
  BCP_REQUIRE((W * C) % 4 == 0, "bcp_mix_box: W*C must be a multiple of 4");
  const long long n_vec = (long long)N * D * H * W * C / 4;
  BCP_REQUIRE(n_vec < (1LL << 29), "bcp_mix_box: tensor too large (>= 2^31 floats)");
  const long long HW4 = (long long)H * (W / 4);
  if (options().mix_c1 && C == 1 && W % 4 == 0 && HW4 * (W / 4) < (1LL << 32) && (long long)N * D <= 65535) {
    const int W4 = W / 4;
    const unsigned magic = (unsigned)(((1ULL << 32) + W4 - 1) / W4);      // W4 >= 1; W4 == 1: 2^32 does not fit -> h = s below
    const int gx = (int)((HW4 + 255) / 256 > 64 ? 64 : (HW4 + 255) / 256);
    if (W4 > 1) {
      hipLaunchKernelGGL(k_mix_box_c1, dim3(gx, N * D), dim3(256), 0, (hipStream_t)stream, a, b, out, (int)HW4, W4, magic, D, box6[0],
                         box6[0] + box6[3], box6[1], box6[1] + box6[4], box6[2], box6[2] + box6[5]);
      BCP_CHECK_LAUNCH("bcp_mix_box");
      return BCP_OK;
    }
  }
  if (n_vec <= (1LL << 20))
    hipLaunchKernelGGL(k_mix_box<1>, dim3(stream_grid(n_vec, 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, n_vec, D, H,
                       W, C, box6[0], box6[0] + box6[3], box6[1], box6[1] + box6[4], box6[2], box6[2] + box6[5]);
  else
    hipLaunchKernelGGL(k_mix_box<4>, dim3(stream_grid((n_vec + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, n_vec, D, H,
                       W, C, box6[0], box6[0] + box6[3], box6[1], box6[1] + box6[4], box6[2], box6[2] + box6[5]);
  BCP_CHECK_LAUNCH("bcp_mix_box");
  return BCP_OK;
}

extern "C" int bcp_mask_boxes(uint8_t* out, int N, int D, int H, int W, const int* boxes, int K, int complement, void* stream) {
  BCP_REQUIRE(out && (boxes || K == 0), "bcp_mask_boxes: null pointer");
  BCP_REQUIRE(K >= 0 && K <= kMaskBoxesMax, "bcp_mask_boxes: %d boxes, at most %d travel as kernel arguments", K, kMaskBoxesMax);
  BCP_REQUIRE(aligned16(out), "bcp_mask_boxes: out must be 16-B aligned");
  BCP_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "bcp_mask_boxes: bad extents");
  BCP_REQUIRE(W % 4 == 0, "bcp_mask_boxes: W must be a multiple of 4");
  BCP_REQUIRE((long long)N * D <= 65535 && (long long)N * D * H * W < (1LL << 31), "bcp_mask_boxes: tensor too large");
  MaskBoxes bx{};
  const int ext[3] = {D, H, W};
  for (int k = 0; k < K; ++k) {
    const int* b = boxes + 6 * k;
    BCP_REQUIRE(b[3] >= 0 && b[4] >= 0 && b[5] >= 0, "bcp_mask_boxes: box %d has a negative size", k);
    bool empty = false;
    int lim[6];
    for (int ax = 0; ax < 3; ++ax) {  // clamp [start, start + size) to [0, extent)
      const long long lo = b[ax] < 0 ? 0 : b[ax], hi = (long long)b[ax] + b[3 + ax] > ext[ax] ? ext[ax] : (long long)b[ax] + b[3 + ax];
      lim[2 * ax] = (int)(lo > ext[ax] ? ext[ax] : lo);
      lim[2 * ax + 1] = (int)hi;
      empty |= lim[2 * ax] >= lim[2 * ax + 1];
    }
    if (empty) continue;
    for (int j = 0; j < 6; ++j) bx.b[bx.k][j] = lim[j];
    ++bx.k;
  }
  const int W16 = (W + 15) / 16;
  const long long items = (long long)H * W16;
  const int gx = (int)((items + 255) / 256 > 64 ? 64 : (items + 255) / 256);
  const unsigned flip = complement ? 0u : 0x01010101u;
  if (W % 16 == 0)
    hipLaunchKernelGGL(k_mask_boxes<true>, dim3(gx, N * D), dim3(256), 0, (hipStream_t)stream, out, D, H, W, W16, bx, flip);
  else
    hipLaunchKernelGGL(k_mask_boxes<false>, dim3(gx, N * D), dim3(256), 0, (hipStream_t)stream, out, D, H, W, W16, bx, flip);
  BCP_CHECK_LAUNCH("bcp_mask_boxes");
  return BCP_OK;
}

extern "C" int bcp_mix_mask(const float* a, const float* b, const uint8_t* mask, float* out, int N, int D, int H, int W,
                            long long mask_sample_stride, void* stream) {
  BCP_REQUIRE(a && b && mask && out, "bcp_mix_mask: null pointer");
  BCP_REQUIRE(aligned16(a) && aligned16(b) && aligned16(out), "bcp_mix_mask: pointers must be 16-B aligned");
  BCP_REQUIRE((reinterpret_cast<uintptr_t>(mask) & 3u) == 0, "bcp_mix_mask: mask must be 4-B aligned");
  BCP_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "bcp_mix_mask: bad extents");
  BCP_REQUIRE(W % 4 == 0, "bcp_mix_mask: W must be a multiple of 4");
  const long long V = (long long)D * H * W, n_vec = (long long)N * V / 4;
  BCP_REQUIRE(n_vec < (1LL << 29) && N <= 65535, "bcp_mix_mask: tensor too large (>= 2^31 floats)");
  BCP_REQUIRE(mask_sample_stride == 0 || (mask_sample_stride >= V && mask_sample_stride % 4 == 0),
              "bcp_mix_mask: mask_sample_stride must be 0 (one map for all samples) or a multiple of 4 >= D*H*W");
  const long long V4 = V / 4;
  long long gx = (V4 + 255) / 256, cap = (2048 + N - 1) / N;      // ~8 workgroups per CU over the whole launch, grid-stride the rest
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL(k_mix_mask, dim3((int)gx, N), dim3(256), 0, (hipStream_t)stream, a, b, mask, out, (int)V4, mask_sample_stride);
  BCP_CHECK_LAUNCH("bcp_mix_mask");
  return BCP_OK;
}

extern "C" int bcp_plabel_bin(const float* logits, uint8_t* out, long long n_vox, float thres, void* stream) {
  BCP_REQUIRE(logits && out, "bcp_plabel_bin: null pointer");
  BCP_REQUIRE(n_vox > 0 && n_vox % 4 == 0, "bcp_plabel_bin: n_vox must be a positive multiple of 4");
  BCP_REQUIRE(aligned16(logits) && (reinterpret_cast<uintptr_t>(out) & 3u) == 0, "bcp_plabel_bin: alignment");
  hipLaunchKernelGGL(k_plabel_bin, dim3(stream_grid(n_vox / 4, 256)), dim3(256), 0, (hipStream_t)stream, logits, out,
                     n_vox / 4, thres);
  BCP_CHECK_LAUNCH("bcp_plabel_bin");
  return BCP_OK;
}

extern "C" int bcp_plabel_argmax4(const float* logits, uint8_t* out, long long n_pix, void* stream) {
  BCP_REQUIRE(logits && out && n_pix > 0, "bcp_plabel_argmax4: bad argument");
  BCP_REQUIRE(aligned16(logits), "bcp_plabel_argmax4: alignment");
  hipLaunchKernelGGL(k_plabel_argmax4, dim3(stream_grid(n_pix, 256)), dim3(256), 0, (hipStream_t)stream, logits, out,
                     n_pix);
  BCP_CHECK_LAUNCH("bcp_plabel_argmax4");
  return BCP_OK;
}

extern "C" int bcp_ema(float* dst, const float* src, long long n, double alpha, void* stream) {
  BCP_REQUIRE(dst && src && n > 0, "bcp_ema: bad argument");
  BCP_REQUIRE(aligned16(dst) && aligned16(src), "bcp_ema: alignment");
  // (1 - alpha) is formed in double then rounded to f32, as python does for (1 - alpha) * tensor
  const float oma = (float)(1.0 - alpha);
  hipLaunchKernelGGL(k_ema, dim3(stream_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, dst, src, n, (float)alpha, oma);
  BCP_CHECK_LAUNCH("bcp_ema");
  return BCP_OK;
}

extern "C" int bcp_sgd(float* p, const float* g, float* buf, float* ema_or_null, long long n, float lr, float momentum,
                       float weight_decay, float grad_scale, int first_step, double ema_alpha, void* stream) {
  BCP_REQUIRE(p && g && buf && n > 0, "bcp_sgd: bad argument");
  const float oma = (float)(1.0 - ema_alpha);
  hipLaunchKernelGGL(k_sgd, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, p, g, buf, ema_or_null, n, lr,
                     momentum, weight_decay, grad_scale, first_step, (float)ema_alpha, oma);
  BCP_CHECK_LAUNCH("bcp_sgd");
  return BCP_OK;
}

extern "C" int bcp_adam(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                        float eps, int step, float grad_scale, void* stream) {
  BCP_REQUIRE(p && g && m && v && n > 0 && step >= 1, "bcp_adam: bad argument");
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(k_adam, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1,
                     beta2, eps, (float)bc1, (float)sqrt(bc2), grad_scale);
  BCP_CHECK_LAUNCH("bcp_adam");
  return BCP_OK;
}

extern "C" int bcp_cast(const void* in, void* out, long long n, int kind, void* stream) {
  BCP_REQUIRE(in && out && n > 0, "bcp_cast: bad argument");
  const dim3 g(stream_grid(n, 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
  switch (kind) {
    case BCP_CAST_I64_U8: hipLaunchKernelGGL(k_i64_to_u8, g, b, 0, s, (const long long*)in, (uint8_t*)out, n); break;
    case BCP_CAST_F32_U8: hipLaunchKernelGGL(k_f32_to_u8, g, b, 0, s, (const float*)in, (uint8_t*)out, n); break;
    case BCP_CAST_U8_F32: hipLaunchKernelGGL(k_u8_to_f32, g, b, 0, s, (const uint8_t*)in, (float*)out, n); break;
    case BCP_CAST_U8_I64: hipLaunchKernelGGL(k_u8_to_i64, g, b, 0, s, (const uint8_t*)in, (long long*)out, n); break;
    default: BCP_REQUIRE(false, "bcp_cast: unknown kind %d", kind);
  }
  BCP_CHECK_LAUNCH("bcp_cast");
  return BCP_OK;
}

extern "C" int bcp_axpy(float* y, const float* x, long long n, float a, void* stream) {
  BCP_REQUIRE(y && x && n > 0, "bcp_axpy: bad argument");
  hipLaunchKernelGGL(k_axpy, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, y, x, n, a);
  BCP_CHECK_LAUNCH("bcp_axpy");
  return BCP_OK;
}

static void bernoulli_launch(void* out, long long n, float p_keep, float keep_value, int as_u8, unsigned long long seed,
                             const unsigned long long* seed_dev, hipStream_t s) {
  const dim3 g(stream_grid(n, 256)), b(256);
  if (as_u8)
    hipLaunchKernelGGL(k_bernoulli_u8, g, b, 0, s, (uint8_t*)out, n, p_keep, (unsigned)seed, (unsigned)(seed >> 32), seed_dev);
  else
    hipLaunchKernelGGL(k_bernoulli_f32, g, b, 0, s, (float*)out, n, p_keep, keep_value, (unsigned)seed, (unsigned)(seed >> 32), seed_dev);
}

extern "C" int bcp_bernoulli(void* out, long long n, float p_keep, float keep_value, int as_u8, unsigned long long seed,
                             void* stream) {
  BCP_REQUIRE(out && n > 0, "bcp_bernoulli: bad argument");
  bernoulli_launch(out, n, p_keep, keep_value, as_u8, seed, nullptr, (hipStream_t)stream);
  BCP_CHECK_LAUNCH("bcp_bernoulli");
  return BCP_OK;
}

extern "C" int bcp_bernoulli_dev(void* out, long long n, float p_keep, float keep_value, int as_u8, const unsigned long long* seed_dev,
                                 void* stream) {
  BCP_REQUIRE(out && n > 0 && seed_dev, "bcp_bernoulli_dev: bad argument");
  bernoulli_launch(out, n, p_keep, keep_value, as_u8, 0ull, seed_dev, (hipStream_t)stream);
  BCP_CHECK_LAUNCH("bcp_bernoulli_dev");
  return BCP_OK;
}

namespace bcp {
struct U64x16 { unsigned long long v[16]; };
__global__ void k_store_u64(unsigned long long* __restrict__ dst, int n, U64x16 vals) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = vals.v[threadIdx.x];
}
}  // namespace bcp

extern "C" int bcp_store_u64(unsigned long long* dst, int n, const unsigned long long* host_values, void* stream) {
  BCP_REQUIRE(dst && host_values && n >= 1 && n <= 16, "bcp_store_u64: 1..16 values (they travel as kernel arguments)");
  bcp::U64x16 v{};
  for (int i = 0; i < n; ++i) v.v[i] = host_values[i];
  hipLaunchKernelGGL(bcp::k_store_u64, dim3(1), dim3(64), 0, (hipStream_t)stream, dst, n, v);
  BCP_CHECK_LAUNCH("bcp_store_u64");
  return BCP_OK;
}
