// bcp_amd/csrc/gnorm.hip -- GroupNorm (+ activation, + Dropout3d channel scale, + residual) forward and backward for channels-last
// activations [N][rows][C] on gfx950.
//
// Reference: normalization='groupnorm' of both V-Net classes, nn.GroupNorm(num_groups=16, num_channels=C) after every conv
// (networks/VNet.py:20-21,49-50,77-78,104-105,131-132, pancreas/Vnet.py:22-23,46-47,73-74).
//
// A group is cg = C / 16 ADJACENT channels of one sample, so every statistic is a sum over whole channels of one sample: the streaming
// passes are those of csrc/norm.hip with one normalisation group per sample (k_col_partial<0 / 1>, k_norm_apply), and what is new is
//   k_gnorm_finalize      per-(sample, channel) fp64 sums -> per-(sample, group) mean / rstd -> the table float[5][N][C] the apply pass and
//                         every table-reading consumer take (mean and rstd repeated over a group's channels; row 4 = mean_c - mean_g)
//   k_gnorm_bwd_finalize  per-(sample, channel) (S1 = sum dz, S2 = sum dz xhat) -> the group means k1, k2 of gamma_c S_c, the parameter
//                         gradients' terms, and the conv-bias gradient in closed form
//   k_gnorm_bwd_apply     dy = scale_c dz - rstd_g (k1_g + xhat k2_g); k_norm_bwd_apply's stream with another last line
// The cg channels of a group are combined inside the 16-lane chunk a finalize workgroup ends with, in channel order, by shuffles: no
// atomics, the same bits on every run.  Built without the SLP vectoriser like the other HBM-bound streams.
#include "common.h"
#include "norm_shared.h"
#include "../../include/bcp_hip.h"

namespace bcp {

// sum of v over the cg lanes of this lane's group, lane g0 first (lanes 0..15 of wave 0 call; cg a power of two <= 16)
__device__ __forceinline__ double group_sum(double v, int g0, int cg) {
  double s = 0.0;
  for (int k = 0; k < cg; ++k) s += __shfl(v, g0 + k);
  return s;
}

// forward finalize: block = (sample n, 16-channel chunk)
__global__ __launch_bounds__(kFinalizeThreads) void k_gnorm_finalize(const double* __restrict__ partial, int nb, int N, int C, int cg,
                                                                     long long rows, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, float eps, float* __restrict__ table,
                                                                     float* __restrict__ amax_out) {
  if (amax_out && blockIdx.x == 0) amax_clear(amax_out);      // the apply pass that follows max-reduces |a| into the slots
  const int chunks = C >> 4;
  const int n = blockIdx.x / chunks, chunk = blockIdx.x % chunks, c = chunk * 16 + (threadIdx.x & 15);
  double s1, s2;
  if (!reduce_partials(partial, nb, C, n, chunk, s1, s2)) return;
  const int g0 = (int)threadIdx.x & ~(cg - 1);
  const double S1 = group_sum(s1, g0, cg), S2 = group_sum(s2, g0, cg);
  const double cnt = (double)cg * (double)rows;
  const double m = S1 / cnt;
  double var = S2 / cnt - m * m;
  if (var < 0.0) var = 0.0;
  const double r = 1.0 / sqrt(var + (double)eps);
  const long long NC = (long long)N * C, idx = (long long)n * C + c;
  const double ga = gamma ? (double)gamma[c] : 1.0, be = beta ? (double)beta[c] : 0.0;
  table[idx] = (float)m;
  table[NC + idx] = (float)r;
  table[2 * NC + idx] = (float)(ga * r);
  table[3 * NC + idx] = (float)be;          // z = (y - mean) * scale + beta, the mean subtracted FIRST as in k_norm_finalize
  table[4 * NC + idx] = (float)(s1 / (double)rows - m);      // the channel's own mean against its group's: sum xhat_c = rows * this * rstd (bias gradient)
}

// backward finalize: block = (sample n, 16-channel chunk).  coef = float[2][N][C] (k1, k2 repeated over a group's channels),
// terms = double[3][N][C]: S1, S2 and the sample's share of the conv-bias gradient
//   sum_voxels dy_c = rstd_g (gamma_c S1_c - rows k1_g - rows k2_g (mean_c - mean_g) rstd_g)
__global__ __launch_bounds__(kFinalizeThreads) void k_gnorm_bwd_finalize(const double* __restrict__ partial, int nb, int N, int C, int cg,
                                                                         long long rows, const float* __restrict__ gamma,
                                                                         const float* __restrict__ table, float* __restrict__ coef,
                                                                         double* __restrict__ terms, float* __restrict__ amax_out) {
  if (amax_out && blockIdx.x == 0) amax_clear(amax_out);      // the apply pass that follows max-reduces |dy| into the slots
  const int chunks = C >> 4;
  const int n = blockIdx.x / chunks, chunk = blockIdx.x % chunks, c = chunk * 16 + (threadIdx.x & 15);
  double s1, s2;
  if (!reduce_partials(partial, nb, C, n, chunk, s1, s2)) return;
  const int g0 = (int)threadIdx.x & ~(cg - 1);
  const double ga = gamma ? (double)gamma[c] : 1.0;
  const double a1 = ga * s1, a2 = ga * s2;
  const double cnt = (double)cg * (double)rows;
  const double k1 = group_sum(a1, g0, cg) / cnt, k2 = group_sum(a2, g0, cg) / cnt;
  const long long NC = (long long)N * C, idx = (long long)n * C + c;
  coef[idx] = (float)k1;
  coef[NC + idx] = (float)k2;
  terms[idx] = s1;
  terms[NC + idx] = s2;
  const double r = (double)table[NC + idx], dev = (double)table[4 * NC + idx];
  terms[2 * NC + idx] = r * (a1 - (double)rows * k1 - (double)rows * k2 * dev * r);
}

// row-reversed position of float4 index p inside a sample (same column): (rows-1-r)*C4 + col
#define GN_REV(p) (nv - C4 - (p) + 2 * col)
// dy = scale_c * dz - rstd_g * (k1_g + xhat * k2_g),  dz = da * chan_scale * act'(z).  blockIdx.y = sample; back to front, as k_norm_bwd_apply
__global__ __launch_bounds__(256) void k_gnorm_bwd_apply(const float* __restrict__ y, const float* __restrict__ da,
                                                         const float* __restrict__ table, const float* __restrict__ coef,
                                                         const float* __restrict__ chan_scale, int act, long long rows, int N, int C, int cg,
                                                         float* __restrict__ dy, const double* __restrict__ terms,
                                                         float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dbias,
                                                         int accumulate, float* __restrict__ amax_out) {
  constexpr int U = 4;
  float amax = 0.f;            // max |dy| of what this thread writes: the fp16 pre-scale of the dgrad / weight-gradient kernels that read dy
  const long long NC = (long long)N * C;
  if (blockIdx.x == 0 && blockIdx.y == 0 && (dgamma || dbias)) {   // parameter gradients: the samples in order, in fp64 (deterministic)
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      double gb = 0.0, gg = 0.0, gx = 0.0;
      for (int n = 0; n < N; ++n) {
        gb += terms[(long long)n * C + c];
        gg += terms[NC + (long long)n * C + c];
        gx += terms[2 * NC + (long long)n * C + c];
      }
      if (dgamma) {
        dbeta[c] = (float)((accumulate ? (double)dbeta[c] : 0.0) + gb);
        dgamma[c] = (float)((accumulate ? (double)dgamma[c] : 0.0) + gg);
      }
      // one channel per group: the group mean removes the bias itself and the sum above is rounding noise -- exact zero, as behind BatchNorm
      if (dbias) dbias[c] = (float)((accumulate ? (double)dbias[c] : 0.0) + (cg > 1 ? gx : 0.0));
    }
  }
  const int C4 = C >> 2;
  const int col = threadIdx.x & (C4 - 1);
  const int n = blockIdx.y;
  const long long nv = rows * C4, base = (long long)n * nv;
  const long long stride = (long long)gridDim.x * 256;
  const long long gc = (long long)n * C + col * 4;
  const float4 mu = ld4(table + gc), rs = ld4(table + NC + gc), sc = ld4(table + 2 * NC + gc), sh = ld4(table + 3 * NC + gc);
  const float4 k1 = ld4(coef + gc), k2 = ld4(coef + NC + gc);
  float4 csl = make_float4(1.f, 1.f, 1.f, 1.f);
  if (chan_scale) csl = ld4(chan_scale + gc);
  const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
  const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, rsv[4] = {rs.x, rs.y, rs.z, rs.w};
  const float k1v[4] = {k1.x, k1.y, k1.z, k1.w}, k2v[4] = {k2.x, k2.y, k2.z, k2.w};
  const float cs[4] = {csl.x, csl.y, csl.z, csl.w};
  auto one = [&](long long i, const float4& v, const float4& d4) {
    const float vv[4] = {v.x, v.y, v.z, v.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w};
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float z = (vv[k] - muv[k]) * scv[k] + shv[k];
      const float dz = dd[k] * cs[k] * act_grad(z, act);
      const float xh = (vv[k] - muv[k]) * rsv[k];
      o[k] = scv[k] * dz - rsv[k] * (k1v[k] + xh * k2v[k]);
    }
    st4(dy + i * 4, make_float4(o[0], o[1], o[2], o[3]));
#pragma unroll
    for (int q = 0; q < 4; ++q) { const float t = fabsf(o[q]); amax = (t > amax || t != t) ? t : amax; }
  };
  long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; j + (U - 1) * stride < nv; j += U * stride) {
    float4 v[U], d4[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long i = base + GN_REV(j + u * stride);
      v[u] = ld4(y + i * 4);
      d4[u] = ld4(da + i * 4);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) one(base + GN_REV(j + u * stride), v[u], d4[u]);
  }
  for (; j < nv; j += stride) {
    const long long i = base + GN_REV(j);
    const float4 v = ld4(y + i * 4), d4 = ld4(da + i * 4);
    one(i, v, d4);
  }
  if (amax_out) block_amax_publish(amax, amax_out);
}

// workspace: double partial[N][nb][C][2], double terms[3][N][C], float coef[2][N][C]
static inline size_t gn_partial_doubles(int N, long long rows, int C) { return (size_t)N * per_sample_stat_rows(rows, C) * C * 2; }

static int check_gnorm_args(const char* fn, int N, long long rows, int C, int groups) {
  BCP_REQUIRE(N >= 1 && rows >= 1, "%s: bad extents", fn);
  BCP_REQUIRE(C >= 16 && C <= 256 && (C & (C - 1)) == 0, "%s: C=%d unsupported (need a power of two in 16..256)", fn, C);
  BCP_REQUIRE(groups >= 1 && C % groups == 0, "%s: C=%d is no multiple of groups=%d", fn, C, groups);
  BCP_REQUIRE(groups == 16 && C / groups <= 16, "%s: groups=%d, C/groups=%d unsupported (need 16 groups of 1, 2, 4, 8 or 16 channels)", fn, groups,
              C / groups);
  return BCP_OK;
}

}  // namespace bcp

using namespace bcp;

extern "C" size_t bcp_gnorm_workspace_bytes(int N, long long rows_per_sample, int C) {
  if (N < 1 || C < 16 || C > 256 || (C & (C - 1)) != 0 || rows_per_sample < 1) return 0;      // the range bcp_gnorm_fwd / _bwd serve
  return (gn_partial_doubles(N, rows_per_sample, C) + (size_t)3 * N * C) * sizeof(double) + (size_t)2 * N * C * sizeof(float);
}

extern "C" int bcp_gnorm_fwd(const float* y, int N, long long rows_per_sample, int C, int groups, const float* gamma, const float* beta, float eps,
                             int act, const float* chan_scale, const float* residual, float* stats, void* workspace, const double* partial_in,
                             int nb_in, float* out, float* amax_out, void* stream) {
  if (int rc = check_gnorm_args("bcp_gnorm_fwd", N, rows_per_sample, C, groups)) return rc;
  BCP_REQUIRE(y && stats && workspace, "bcp_gnorm_fwd: null pointer");
  BCP_REQUIRE(aligned16(y) && (!out || aligned16(out)) && aligned16(stats) && aligned16(workspace) && (!residual || aligned16(residual)) &&
                  (!chan_scale || aligned16(chan_scale)),
              "bcp_gnorm_fwd: alignment");
  BCP_REQUIRE(out || !residual, "bcp_gnorm_fwd: statistics-only mode (out = NULL) takes no residual");
  BCP_REQUIRE(!partial_in || (nb_in > 0 && (reinterpret_cast<uintptr_t>(partial_in) & 7u) == 0), "bcp_gnorm_fwd: partial_in needs nb_in > 0 and 8-byte alignment");
  hipStream_t s = (hipStream_t)stream;
  const int cg = C / groups;
  double* partial = reinterpret_cast<double*>(workspace);
  int nb = nb_in;
  if (!partial_in) {
    per_sample_stats_launch(y, N, rows_per_sample, C, partial, s);
    nb = per_sample_stat_rows(rows_per_sample, C);
  }
  hipLaunchKernelGGL(k_gnorm_finalize, dim3(N * (C / 16)), dim3(kFinalizeThreads), 0, s, partial_in ? partial_in : partial, nb, N, C, cg, rows_per_sample,
                     gamma, beta, eps, stats, out ? amax_out : (float*)nullptr);
  if (out) per_sample_apply_launch(y, stats, N, rows_per_sample, C, act, chan_scale, residual, out, amax_out, s);
  BCP_CHECK_LAUNCH("bcp_gnorm_fwd");
  return BCP_OK;
}

extern "C" int bcp_gnorm_bwd(const float* y, const float* da, int N, long long rows_per_sample, int C, int groups, const float* stats,
                             const float* gamma, int act, const float* chan_scale, float* dgamma, float* dbeta, float* dbias, int accumulate,
                             void* workspace, const double* partial_in, int nb_in, float* dy, float* amax_out, void* stream) {
  if (int rc = check_gnorm_args("bcp_gnorm_bwd", N, rows_per_sample, C, groups)) return rc;
  BCP_REQUIRE(y && da && stats && workspace && dy, "bcp_gnorm_bwd: null pointer");
  BCP_REQUIRE(aligned16(y) && aligned16(da) && aligned16(dy) && aligned16(stats) && aligned16(workspace) && (!chan_scale || aligned16(chan_scale)),
              "bcp_gnorm_bwd: alignment");
  BCP_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "bcp_gnorm_bwd: dgamma and dbeta come as a pair");
  BCP_REQUIRE(!partial_in || (nb_in > 0 && !chan_scale && (reinterpret_cast<uintptr_t>(partial_in) & 7u) == 0),
              "bcp_gnorm_bwd: partial_in needs nb_in > 0, 8-byte alignment and no dropout epilogue");
  hipStream_t s = (hipStream_t)stream;
  const int cg = C / groups;
  double* partial = reinterpret_cast<double*>(workspace);
  double* terms = partial + gn_partial_doubles(N, rows_per_sample, C);
  float* coef = reinterpret_cast<float*>(terms + (size_t)3 * N * C);
  int nb = nb_in;
  if (!partial_in) {
    per_sample_bwd_stats_launch(y, da, stats, N, rows_per_sample, C, act, chan_scale, partial, s);
    nb = per_sample_stat_rows(rows_per_sample, C);
  }
  hipLaunchKernelGGL(k_gnorm_bwd_finalize, dim3(N * (C / 16)), dim3(kFinalizeThreads), 0, s, partial_in ? partial_in : partial, nb, N, C, cg,
                     rows_per_sample, gamma, stats, coef, terms, amax_out);
  hipLaunchKernelGGL(k_gnorm_bwd_apply, dim3(per_sample_apply_blocks(rows_per_sample, C, N), N), dim3(256), 0, s, y, da, stats, coef, chan_scale, act,
                     rows_per_sample, N, C, cg, dy, terms, dgamma, dbeta, dbias, accumulate, amax_out);
  BCP_CHECK_LAUNCH("bcp_gnorm_bwd");
  return BCP_OK;
}
