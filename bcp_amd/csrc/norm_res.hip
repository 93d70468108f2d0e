// bcp_amd/csrc/norm_res.hip -- BatchNorm (train / eval) + activation with a PRE-activation residual, forward and backward, for channels-last
// activations [rows][C] on gfx950: the closing layer of the reference's ResidualConvBlock (networks/VNet.py:35-65, has_residual=True),
//
//     a = act((y - mean) * scale + shift + r) [* chan_scale]            r = the block's input: [rows][C], or [rows][1] broadcast (block_one)
//
// csrc/norm.hip's passes add their residual BEHIND the activation (the decoder's skip add) and rebuild the activation pattern from z alone;
// here the pattern is that of z + r, both backward passes read r, and the apply pass also leaves dres = g = da * chan_scale * act'(z + r),
// the gradient of the block input through the shortcut.  The statistics of y are norm.hip's (its statistics pass, or the rows a *_fwd_stats
// epilogue left) and so are the finalize kernels: only the streams that touch r are new.  Same shape as norm.hip's streams -- a thread owns
// one float4 channel group, four loads in flight per operand, the apply passes walk back to front, one |max| publish per workgroup -- as
// kernels of their own (template instances on the residual's width), so the existing launches keep their bits.
#include "common.h"
#include "norm_shared.h"
#include "../../include/bcp_hip.h"

namespace bcp {

// the residual of the four channels at float4 index i (row = (i - col) / C4): its own float4, or the row's single value in all four
template <bool RB>
__device__ __forceinline__ float4 ld_res(const float* __restrict__ res, long long i, int col, int c4sh) {
  if (RB) { const float r = res[(i - col) >> c4sh]; return make_float4(r, r, r, r); }
  return ld4(res + i * 4);
}

#define REV(p) (nv - C4 - (p) + 2 * col)      // row-reversed position of float4 index p inside a segment (csrc/norm.hip)

// segments as in csrc/norm.hip: blockIdx.y = one normalisation group, or one sample of it when a per-(sample, channel) scale is present
template <bool RB>
__global__ __launch_bounds__(256) void k_norm_apply_res(const float* __restrict__ y, const float* __restrict__ scale, const float* __restrict__ shift,
                                                        const float* __restrict__ mean, const float* __restrict__ res,
                                                        const float* __restrict__ chan_scale, long long rows_per_sample, int act, long long seg_rows,
                                                        int spg, int C, float* __restrict__ out, float* __restrict__ amax_out) {
  constexpr int U = 4;
  float amax = 0.f;
  const int C4 = C >> 2;
  const int c4sh = 31 - __clz(C4);
  const int col = threadIdx.x & (C4 - 1);
  const int seg = blockIdx.y, g = seg / spg;
  const long long nv = seg_rows * C4, base = (long long)seg * nv;
  const long long stride = (long long)gridDim.x * 256;
  const float4 sc = ld4(scale + (long long)g * C + col * 4), sh = ld4(shift + (long long)g * C + col * 4);
  const float4 mu = ld4(mean + (long long)g * C + col * 4);
  float4 cs = make_float4(1.f, 1.f, 1.f, 1.f);
  if (chan_scale) cs = ld4(chan_scale + (((long long)seg * seg_rows) / rows_per_sample) * C + col * 4);
  auto one = [&](long long i, const float4& v, const float4& r4) {
    float o[4] = {act_fwd(((v.x - mu.x) * sc.x + sh.x) + r4.x, act), act_fwd(((v.y - mu.y) * sc.y + sh.y) + r4.y, act),
                  act_fwd(((v.z - mu.z) * sc.z + sh.z) + r4.z, act), act_fwd(((v.w - mu.w) * sc.w + sh.w) + r4.w, act)};
    if (chan_scale) { o[0] *= cs.x; o[1] *= cs.y; o[2] *= cs.z; o[3] *= cs.w; }
    st4(out + i * 4, make_float4(o[0], o[1], o[2], o[3]));
#pragma unroll
    for (int k = 0; k < 4; ++k) { const float t = fabsf(o[k]); amax = (t > amax || t != t) ? t : amax; }
  };
  long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; j + (U - 1) * stride < nv; j += U * stride) {
    float4 v[U], r4[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long i = base + REV(j + u * stride);
      v[u] = ld4(y + i * 4);
      r4[u] = ld_res<RB>(res, i, col, c4sh);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) one(base + REV(j + u * stride), v[u], r4[u]);
  }
  for (; j < nv; j += stride) {
    const long long i = base + REV(j);
    const float4 v = ld4(y + i * 4), r4 = ld_res<RB>(res, i, col, c4sh);
    one(i, v, r4);
  }
  if (amax_out) block_amax_publish(amax, amax_out);
}

// (sum g, sum g * xhat) per (group, block, channel), g = da * chan_scale * act'(z + r): csrc/norm.hip's k_col_partial<1> with the pattern of
// z + r; same partial-row layout [G][spg * gridDim.x][C][2], same reduction over the row slots
template <bool RB>
__global__ __launch_bounds__(256) void k_col_partial_res(const float* __restrict__ y, const float* __restrict__ da, const float* __restrict__ res,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ chan_scale, long long rows_per_sample, int act,
                                                         long long seg_rows, int spg, int C, double* __restrict__ partial) {
  constexpr int U = 4;
  const int C4 = C >> 2;
  const int col = threadIdx.x % C4;
  const int slot = threadIdx.x / C4;
  const int slots = 256 / C4;
  const int seg = blockIdx.y, g = seg / spg, nbps = gridDim.x;
  const long long chunk = (seg_rows + nbps - 1) / nbps;
  const long long r0 = (long long)blockIdx.x * chunk;
  long long r1 = r0 + chunk;
  if (r1 > seg_rows) r1 = seg_rows;
  const long long sbase = (long long)seg * seg_rows;
  double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  const long long gc = (long long)g * C + col * 4;
  const float4 sc = ld4(scale + gc), sh = ld4(shift + gc), mu = ld4(mean + gc), rs = ld4(rstd + gc);
  const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
  const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, rsv[4] = {rs.x, rs.y, rs.z, rs.w};
  float csv[4] = {1.f, 1.f, 1.f, 1.f};
  if (chan_scale) {
    const float4 c4 = ld4(chan_scale + (sbase / rows_per_sample) * C + col * 4);
    csv[0] = c4.x; csv[1] = c4.y; csv[2] = c4.z; csv[3] = c4.w;
  }
  auto accum = [&](const float4& v, const float4& d4, const float4& r4) {
    const float vv[4] = {v.x, v.y, v.z, v.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w}, rr[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float t = ((vv[k] - muv[k]) * scv[k] + shv[k]) + rr[k];
      const float g1 = dd[k] * csv[k] * act_grad(t, act);
      const float xh = (vv[k] - muv[k]) * rsv[k];
      s1[k] += (double)g1;
      s2[k] += (double)g1 * (double)xh;
    }
  };
  auto ldr = [&](long long row) -> float4 {
    if (RB) { const float r = res[row]; return make_float4(r, r, r, r); }
    return ld4(res + (row * C4 + col) * 4);
  };
  if (slot < slots) {
    long long r = r0 + slot;
    for (; r + (long long)(U - 1) * slots < r1; r += (long long)U * slots) {
      float4 v[U], d4[U], r4[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long row = sbase + r + (long long)u * slots;
        const long long e = (row * C4 + col) * 4;
        v[u] = ld4(y + e);
        d4[u] = ld4(da + e);
        r4[u] = ldr(row);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) accum(v[u], d4[u], r4[u]);
    }
    for (; r < r1; r += slots) {
      const long long row = sbase + r;
      const long long e = (row * C4 + col) * 4;
      accum(ld4(y + e), ld4(da + e), ldr(row));
    }
  }
  // block reduce over the row slots: xor-shuffles inside a wave (lanes with equal column are C4 apart), then one LDS hop over the waves
  double acc8[8] = {s1[0], s1[1], s1[2], s1[3], s2[0], s2[1], s2[2], s2[3]};
  for (int off = C4; off < 64; off <<= 1) {
#pragma unroll
    for (int k = 0; k < 8; ++k) acc8[k] += __shfl_xor(acc8[k], off);
  }
  __shared__ double red[4][64][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool leader = (C4 >= 64) || lane < C4;
  if (leader) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[wave][lane][k] = acc8[k];
  }
  __syncthreads();
  if ((int)threadIdx.x < C4) {
    // C4 <= 64: column col lives at lane col of every wave.  C4 = 128 / 256: column col lives in wave (col / 64) + j * (C4 / 64)
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int wpr = C4 >= 64 ? C4 / 64 : 1;
    const int w0 = C4 >= 64 ? col / 64 : 0;
    for (int w = w0; w < 4; w += wpr) {
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] += red[w][col & 63][k];
    }
    const long long prow = (long long)g * spg * nbps + (long long)(seg - g * spg) * nbps + blockIdx.x;
    double* po = partial + (prow * C + col * 4) * 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) { po[k * 2] = a[k]; po[k * 2 + 1] = a[4 + k]; }
  }
}

// dy = scale * (g - c1 - xhat * c2),  dres = g  (nullable),  g = da * chan_scale * act'(z + r)
template <bool RB>
__global__ __launch_bounds__(256) void k_norm_bwd_apply_res(const float* __restrict__ y, const float* __restrict__ da, const float* __restrict__ res,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ c1, const float* __restrict__ c2,
                                                            const float* __restrict__ chan_scale, long long rows_per_sample, int act,
                                                            long long seg_rows, int spg, int C, float* __restrict__ dy, float* __restrict__ dres,
                                                            float* __restrict__ amax_out) {
  constexpr int U = 4;
  float amax = 0.f;
  const int C4 = C >> 2;
  const int c4sh = 31 - __clz(C4);
  const int col = threadIdx.x & (C4 - 1);
  const int seg = blockIdx.y, g = seg / spg;
  const long long nv = seg_rows * C4, base = (long long)seg * nv;
  const long long stride = (long long)gridDim.x * 256;
  const long long gc = (long long)g * C + col * 4;
  const float4 sc = ld4(scale + gc), sh = ld4(shift + gc), mu = ld4(mean + gc), rs = ld4(rstd + gc);
  const float4 k1 = ld4(c1 + gc), k2 = ld4(c2 + gc);
  float4 csl = make_float4(1.f, 1.f, 1.f, 1.f);
  if (chan_scale) csl = ld4(chan_scale + (((long long)seg * seg_rows) / rows_per_sample) * C + col * 4);
  const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
  const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, rsv[4] = {rs.x, rs.y, rs.z, rs.w};
  const float k1v[4] = {k1.x, k1.y, k1.z, k1.w}, k2v[4] = {k2.x, k2.y, k2.z, k2.w};
  const float csv[4] = {csl.x, csl.y, csl.z, csl.w};
  auto one = [&](long long i, const float4& v, const float4& d4, const float4& r4) {
    const float vv[4] = {v.x, v.y, v.z, v.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w}, rr[4] = {r4.x, r4.y, r4.z, r4.w};
    float o[4], gq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float t = ((vv[k] - muv[k]) * scv[k] + shv[k]) + rr[k];
      gq[k] = dd[k] * csv[k] * act_grad(t, act);
      const float xh = (vv[k] - muv[k]) * rsv[k];
      o[k] = scv[k] * (gq[k] - k1v[k] - xh * k2v[k]);
    }
    st4(dy + i * 4, make_float4(o[0], o[1], o[2], o[3]));
    if (dres) st4(dres + i * 4, make_float4(gq[0], gq[1], gq[2], gq[3]));
#pragma unroll
    for (int q = 0; q < 4; ++q) { const float t = fabsf(o[q]); amax = (t > amax || t != t) ? t : amax; }
  };
  long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; j + (U - 1) * stride < nv; j += U * stride) {
    float4 v[U], d4[U], r4[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long i = base + REV(j + u * stride);
      v[u] = ld4(y + i * 4);
      d4[u] = ld4(da + i * 4);
      r4[u] = ld_res<RB>(res, i, col, c4sh);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) one(base + REV(j + u * stride), v[u], d4[u], r4[u]);
  }
  for (; j < nv; j += stride) {
    const long long i = base + REV(j);
    const float4 v = ld4(y + i * 4), d4 = ld4(da + i * 4), r4 = ld_res<RB>(res, i, col, c4sh);
    one(i, v, d4, r4);
  }
  if (amax_out) block_amax_publish(amax, amax_out);
}

// eval-mode BatchNorm (running statistics, no update): csrc/eval.hip's k_norm_eval with the residual in front of the activation
template <bool RB>
__global__ __launch_bounds__(256) void k_norm_eval_res(const float* __restrict__ y, long long rows, int C, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ rmean,
                                                       const float* __restrict__ rvar, float eps, int act, const float* __restrict__ res,
                                                       float* __restrict__ out) {
  const int C4 = C >> 2;
  const int c4sh = 31 - __clz(C4);
  const int col = threadIdx.x & (C4 - 1);
  const float4 mu = ld4(rmean + col * 4), va = ld4(rvar + col * 4);
  float4 ga = make_float4(1.f, 1.f, 1.f, 1.f), be = make_float4(0.f, 0.f, 0.f, 0.f);
  if (gamma) ga = ld4(gamma + col * 4);
  if (beta) be = ld4(beta + col * 4);
  // torch: invstd = 1 / sqrt(var + eps) in fp32, then (x - mean) * invstd * weight + bias
  const float sx = ga.x * (1.f / sqrtf(va.x + eps)), sy = ga.y * (1.f / sqrtf(va.y + eps));
  const float sz = ga.z * (1.f / sqrtf(va.z + eps)), sw = ga.w * (1.f / sqrtf(va.w + eps));
  const long long nv = rows * C4, stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
    const float4 v = ld4(y + i * 4), r4 = ld_res<RB>(res, i, col, c4sh);
    st4(out + i * 4, make_float4(act_fwd(((v.x - mu.x) * sx + be.x) + r4.x, act), act_fwd(((v.y - mu.y) * sy + be.y) + r4.y, act),
                                 act_fwd(((v.z - mu.z) * sz + be.z) + r4.z, act), act_fwd(((v.w - mu.w) * sw + be.w) + r4.w, act)));
  }
}

// the instances by the residual's width: [res_channels == 1]
static const decltype(&k_norm_apply_res<false>) kApplyRes[2] = {k_norm_apply_res<false>, k_norm_apply_res<true>};
static const decltype(&k_col_partial_res<false>) kColPartialRes[2] = {k_col_partial_res<false>, k_col_partial_res<true>};
static const decltype(&k_norm_bwd_apply_res<false>) kBwdApplyRes[2] = {k_norm_bwd_apply_res<false>, k_norm_bwd_apply_res<true>};
static const decltype(&k_norm_eval_res<false>) kEvalRes[2] = {k_norm_eval_res<false>, k_norm_eval_res<true>};

// norm_problem() and the residual's own checks
static int res_problem(const char* fn, int G, long long rows_per_group, int C, const float* chan_scale, long long rows_per_sample, int act, const float* res,
                       int res_channels, NormProblem& p) {
  if (int rc = norm_problem(fn, G, rows_per_group, C, NormEpilogue{chan_scale, nullptr, 1.f, rows_per_sample, act, nullptr, 0.f}, p)) return rc;
  BCP_REQUIRE(res != nullptr, "%s: null residual (bcp_norm_fwd / _bwd / _eval are the entry points without one)", fn);
  BCP_REQUIRE(res_channels == C || res_channels == 1, "%s: res_channels=%d (need C=%d, or 1 for a broadcast residual)", fn, res_channels, C);
  BCP_REQUIRE(res_channels == 1 ? (reinterpret_cast<uintptr_t>(res) & 3u) == 0 : aligned16(res), "%s: alignment of the residual", fn);
  return BCP_OK;
}

}  // namespace bcp

using namespace bcp;

extern "C" int bcp_norm_fwd_res(const float* y, int G, long long rows_per_group, int C, const float* gamma, const float* beta, float* running_mean,
                                float* running_var, float momentum, float eps, int act, const float* chan_scale, long long rows_per_sample,
                                const float* res_pre, int res_channels, float* stats, void* workspace, const double* partial_in, int nb_in,
                                float* out, float* amax_out, void* stream) {
  BCP_REQUIRE(out != nullptr, "bcp_norm_fwd_res: statistics-only mode (out = NULL) takes no residual: use bcp_norm_fwd");
  NormProblem p;
  if (int rc = res_problem("bcp_norm_fwd_res", G, rows_per_group, C, chan_scale, rows_per_sample, act, res_pre, res_channels, p)) return rc;
  BCP_REQUIRE(y && stats && workspace, "bcp_norm_fwd_res: null pointer");
  BCP_REQUIRE(aligned16(y) && aligned16(out) && aligned16(stats) && aligned16(workspace) && (!chan_scale || aligned16(chan_scale)) &&
                  (!gamma || aligned16(gamma)) && (!beta || aligned16(beta)), "bcp_norm_fwd_res: alignment");
  BCP_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bcp_norm_fwd_res: running_mean and running_var come together");
  BCP_REQUIRE(!partial_in || nb_in > 0, "bcp_norm_fwd_res: partial_in without rows");
  hipStream_t s = (hipStream_t)stream;
  const NormRoute r = norm_route(NormDir::Fwd, partial_in ? NormSrc::Partial : NormSrc::Tensor, p, true, running_mean != nullptr);
  const NormTable t = norm_table(stats, G, C);
  // statistics of y: norm.hip's pass (one partial-row block per group), or the producer's rows; finalize (clears the |max| slots) + running statistics
  double* partial = reinterpret_cast<double*>(workspace);
  if (!partial_in) per_sample_stats_launch(y, G, rows_per_group, C, partial, s);
  norm_fwd_finalize_launch(partial_in ? partial_in : partial, partial_in ? nb_in : per_sample_stat_rows(rows_per_group, C), G, C, rows_per_group, gamma, beta,
                           running_mean, running_var, momentum, eps, stats, s, amax_out);
  hipLaunchKernelGGL(kApplyRes[res_channels == 1], r.apply_grid, dim3(256), 0, s, y, t.scale, t.shift, t.mean, res_pre,
                     chan_scale, p.ep.rows_per_sample, act, p.seg_rows, p.spg, C, out, amax_out);
  BCP_CHECK_LAUNCH("bcp_norm_fwd_res");
  return BCP_OK;
}

extern "C" int bcp_norm_bwd_res(const float* y, const float* da, const float* res_pre, int res_channels, int G, long long rows_per_group, int C,
                                const float* stats, int act, const float* chan_scale, long long rows_per_sample, float* dgamma, float* dbeta,
                                int accumulate, void* workspace, float* dy, float* dres, float* amax_out, void* stream) {
  NormProblem p;
  if (int rc = res_problem("bcp_norm_bwd_res", G, rows_per_group, C, chan_scale, rows_per_sample, act, res_pre, res_channels, p)) return rc;
  BCP_REQUIRE(y && da && stats && workspace && dy, "bcp_norm_bwd_res: null pointer");
  BCP_REQUIRE(aligned16(y) && aligned16(da) && aligned16(stats) && aligned16(workspace) && aligned16(dy) && (!dres || aligned16(dres)) &&
                  (!chan_scale || aligned16(chan_scale)), "bcp_norm_bwd_res: alignment");
  BCP_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "bcp_norm_bwd_res: dgamma and dbeta come together");
  BCP_REQUIRE(!(dres && res_channels == 1), "bcp_norm_bwd_res: the gradient of a broadcast residual is not produced (dres must be NULL for res_channels = 1)");
  hipStream_t s = (hipStream_t)stream;
  // the chain of bcp_norm_bwd over the tensor, with the streams that read r: its grids, its partial rows and its c1c2raw behind them
  const NormRoute r = norm_route(NormDir::Bwd, NormSrc::Tensor, p, true, dgamma != nullptr);
  const NormTable t = norm_table(stats, G, C);
  double* partial = reinterpret_cast<double*>(workspace);
  const NormCoef k = norm_coef(reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + r.c1_offset), G, C);
  const int rb = res_channels == 1;
  hipLaunchKernelGGL(kColPartialRes[rb], r.stat_grid, dim3(256), 0, s, y, da, res_pre, t.scale, t.shift, t.mean,
                     t.rstd, chan_scale, p.ep.rows_per_sample, act, p.seg_rows, p.spg, C, partial);
  norm_bwd_finalize_launch(partial, r.nb, G, C, rows_per_group, dgamma, dbeta, accumulate, k.c1, s, amax_out);
  hipLaunchKernelGGL(kBwdApplyRes[rb], r.apply_grid, dim3(256), 0, s, y, da, res_pre, t.scale, t.shift, t.mean,
                     t.rstd, k.c1, k.c2, chan_scale, p.ep.rows_per_sample, act, p.seg_rows, p.spg, C, dy, dres, amax_out);
  BCP_CHECK_LAUNCH("bcp_norm_bwd_res");
  return BCP_OK;
}

extern "C" int bcp_norm_eval_res(const float* y, long long rows, int C, const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, float eps, int act, const float* res_pre, int res_channels, float* out, void* stream) {
  NormProblem p;
  if (int rc = res_problem("bcp_norm_eval_res", 1, rows, C, nullptr, 0, act, res_pre, res_channels, p)) return rc;
  BCP_REQUIRE(y && running_mean && running_var && out, "bcp_norm_eval_res: null pointer");
  BCP_REQUIRE(aligned16(y) && aligned16(out) && aligned16(running_mean) && aligned16(running_var) && (!gamma || aligned16(gamma)) && (!beta || aligned16(beta)),
              "bcp_norm_eval_res: alignment");
  const long long nvec = rows * (C / 4);
  long long gx = (nvec + 255) / 256;
  if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(kEvalRes[res_channels == 1], dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, y, rows, C, gamma, beta, running_mean, running_var, eps, act,
                     res_pre, out);
  BCP_CHECK_LAUNCH("bcp_norm_eval_res");
  return BCP_OK;
}

