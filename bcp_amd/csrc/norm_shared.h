// bcp_amd/csrc/norm_shared.h -- what csrc/norm.hip (BatchNorm / InstanceNorm) shares with csrc/norm_res.hip (pre-activation residual) and
// csrc/gnorm.hip (GroupNorm): the problem record of the family's host dispatch, the views of its two tables, the reduction of the
// per-block fp64 partial rows, and host launchers for the finalize steps and the per-sample statistics / apply streams.
#pragma once
#include "common.h"

namespace bcp {

struct NormEpilogue {
  const float* chan_scale;     // nullable [N][C]: Dropout3d keep*1/(1-p) per (sample, channel)
  const uint8_t* elem_mask;    // nullable [rows][C]: elementwise Dropout keep mask
  float elem_scale;            // 1/(1-p) for elem_mask
  long long rows_per_sample;   // spatial size (rows per n) for chan_scale indexing
  int act;
  const unsigned long long* mask_seed;   // nullable (round 4): device seed of an elementwise Dropout whose keep bits are EVALUATED here
  float p_keep;                          //   (bern_keep, common.h: the bits bcp_bernoulli_dev would write) instead of read from elem_mask
};

// ---- the problem record of the host dispatch (csrc/norm.hip norm_route() decides from it, norm_fwd_launch() / norm_bwd_launch() launch it).
// Segments (see k_col_partial): the finer of (group, sample) when a per-sample channel scale is present -- spg of them per group
constexpr int kMaxSamplesPerGroup = 64;      // (bcp_norm_workspace_bytes leaves room for this many more partial rows per group)
struct NormProblem { int G; long long rows_per_group; int C; NormEpilogue ep; long long seg_rows; int spg; };
// checks the extents, C (a power of two in 16 .. 1024) and that a group holds 1 .. kMaxSamplesPerGroup whole samples under a channel
// scale; ep.rows_per_sample <= 0 stands for rows_per_group
int norm_problem(const char* fn, int G, long long rows_per_group, int C, const NormEpilogue& ep, NormProblem& p);

// the statistics table float[5][G][C] and the backward coefficients c1c2raw = float[4][G][C] (c1, c2, then the two raw sums)
struct NormTable { float *mean, *rstd, *scale, *shift, *var_unb; };
inline NormTable norm_table(const float* stats, int G, int C) {      // (the forward finalize steps are the only writers)
  float* t = const_cast<float*>(stats);
  return {t, t + (long long)G * C, t + 2LL * G * C, t + 3LL * G * C, t + 4LL * G * C};
}
struct NormCoef { float *c1, *c2, *raw; };
inline NormCoef norm_coef(float* c1c2raw, int G, int C) { return {c1c2raw, c1c2raw + (long long)G * C, c1c2raw + 2LL * G * C}; }

// ---- the route: everything the host decides about one call, decided once (csrc/norm.hip norm_route; launch-free and pure)
enum class NormDir { Fwd, Bwd };
enum class NormSrc { Tensor, Slabs, Partial };      // the statistics: a pass over the tensor, a pass that sums split-K slabs on its way in, rows handed in
enum class NormForm { Own, Fused, Chain };          // one launch / statistics pass, apply pass that finalises / statistics pass, finalize, tail
enum class NormTail { None, Apply, Params };        // behind the chain's finalize: the apply pass, or (no output) k_norm_running_only / k_norm_bwd_params
struct NormRoute {
  NormForm form; NormTail tail; bool stats, finalize;      // finalize: the finalize launch happens (stats: the statistics pass)
  int nbps, nseg, nb;                                      // partial rows per segment, segments, partial rows per group
  dim3 stat_grid, fin_grid, apply_grid, fused_grid, own_grid;
  int GS, cw, P;                                           // the one-launch form: groups and channels per workgroup, kernel instance
  bool skip_fin, skip_app, skip_bstat;                     // options().whatif: launches left out to price a change (wrong results)
  int cap_rows; size_t c1_offset;                          // workspace: partial rows per group in front of c1c2raw, its byte offset
};
// has_out: an apply pass writes a tensor (the backward entry points: always); ordered: running statistics / parameter gradients are updated
NormRoute norm_route(NormDir dir, NormSrc src, const NormProblem& p, bool has_out, bool ordered);

// Sum the per-block partials of 16 channels of one group: 1024 threads = 32 doubles (16 channels x {s1, s2}, one 256-byte
// row of the partial table) x 32 row-slots, four independent loads in flight per thread, then an LDS tree.  Threads 0..15
// return true with the two sums of channel chunk*16 + tid.  (A single thread walking ~1000 partials serially cost more than
// the streaming pass itself; 16 slots with one load in flight left this kernel at ~8 us on the step's critical path.)
constexpr int kFinalizeThreads = 1024;
__device__ __forceinline__ bool reduce_partials(const double* __restrict__ partial, int nb, int C, int g, int chunk,
                                                double& s1, double& s2) {
  __shared__ double red[32][33];
  __shared__ double fin[32];
  const int e = threadIdx.x & 31, slot = threadIdx.x >> 5;
  const double* p = partial + ((long long)g * nb * C + chunk * 16) * 2 + e;
  const long long rs = (long long)C * 2;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int b = slot;
  for (; b + 96 < nb; b += 128) {
    const double v0 = p[b * rs], v1 = p[(b + 32) * rs], v2 = p[(b + 64) * rs], v3 = p[(b + 96) * rs];
    a0 += v0; a1 += v1; a2 += v2; a3 += v3;
  }
  for (; b < nb; b += 32) a0 += p[b * rs];
  red[slot][e] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (threadIdx.x < 32) {
    double t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int k = 0; k < 32; k += 2) { t0 += red[k][e]; t1 += red[k + 1][e]; }
    fin[e] = t0 + t1;
  }
  __syncthreads();
  if (threadIdx.x >= 16) return false;
  s1 = fin[threadIdx.x * 2];
  s2 = fin[threadIdx.x * 2 + 1];
  return true;
}

// ---- the finalize kernels of csrc/norm.hip behind a statistics pass that somebody else made (csrc/gemm.hip bcp_up_fwd_norm / bcp_up_norm_bwd):
// partial[G][nb][C][2] -> the statistics table float[5][G][C] (and the running statistics) / dgamma, dbeta and c1c2raw = float[4][G][C]
void norm_fwd_finalize_launch(const double* partial, int nb, int G, int C, long long rows_per_group, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, float momentum, float eps, float* stats, hipStream_t s, float* amax_clear_or_null);
void norm_bwd_finalize_launch(const double* partial, int nb, int G, int C, long long rows_per_group, float* dgamma, float* dbeta, int accumulate,
                              float* c1c2raw, hipStream_t s, float* amax_clear_or_null);

// ---- per-sample streams of csrc/norm.hip launched for a GroupNorm layer (groups of the streams = samples; table = float[5][N][C])
// partial rows per sample the statistics passes below leave (the workspace holds N x this many rows of [C][2] doubles)
int per_sample_stat_rows(long long rows_per_sample, int C);
// k_col_partial<0>: (sum y, sum y^2) per (sample, block, channel)
void per_sample_stats_launch(const float* y, int N, long long rows_per_sample, int C, double* partial, hipStream_t s);
// k_col_partial<1>: (sum dz, sum dz * xhat) per (sample, block, channel), xhat and the activation pattern from the table
void per_sample_bwd_stats_launch(const float* y, const float* da, const float* table, int N, long long rows_per_sample, int C, int act,
                                 const float* chan_scale, double* partial, hipStream_t s);
// k_norm_apply: a = act((y - mean) * scale + shift) [* chan_scale] [+ residual], |max| of a into amax_out's slots
void per_sample_apply_launch(const float* y, const float* table, int N, long long rows_per_sample, int C, int act, const float* chan_scale,
                             const float* residual, float* out, float* amax_out, hipStream_t s);
// the grid the apply passes are sized for (norm_apply_cap / norm_apply_vec options included)
int per_sample_apply_blocks(long long rows_per_sample, int C, int N);

}  // namespace bcp
