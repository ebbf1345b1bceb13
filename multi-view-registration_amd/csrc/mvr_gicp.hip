// csrc/mvr_gicp.hip -- pcl::GeneralizedIterativeClosestPoint's inner optimisation on the GPU (gfx950); the rules G1-G10 are
// written next to mvr_icp_align_gicp in mvr_hip.h.
//
// An evaluation of the plane-to-plane objective is one sweep over the match table the search and the rejector chain left on the
// device: four 16-byte loads per live entry (p, s, q[j], n[j]), some eighty f64 operations, 29 f64 sums.  That is a few
// microseconds of traffic, so what an optimiser costs is the launches and the trips to the host, and the Levenberg-Marquardt
// loop of G7 therefore lives on the device:
//   gicp_sums_kernel   the 29 sums of G5 at the CANDIDATE pose of the state block, block partials in the order of p2plane_kernel;
//   gicp_step_kernel   one block adds the partial rows in fixed order; one thread decides accept / reject (G7), solves the damped
//                      6x6 system (G6) and writes the next candidate, lambda, the counters and `done` into the state block.
// The host queues evaluation + step pairs behind each other and reads the state block once per chunk.  A pair that finds `done`
// set returns at once (every block of the sums launch, and the step's deciding thread), so queuing all max_inner_iterations pairs
// and queuing them one by one give the same bits.
// Compiled with -ffp-contract=off.
#include "mvr_internal.h"
#include "mvr_block_sums.h"

namespace mvr {

namespace {

struct GicpOpt {
  double rot_tol, trans_tol;
  int max_inner;
  int sums_only;         // mvr_gicp_sums: the step kernel only leaves the sums of the one evaluation in the state block
};

struct GicpX { double v[12]; };      // R row-major, then t

__device__ __forceinline__ uint32_t *gicp_words(double *state) { return reinterpret_cast<uint32_t *>(state + kGicpWordsAt); }

__global__ void gicp_init_kernel(double *state, GicpX x)
{
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int k = 0; k < kGicpStateDoubles; ++k) state[k] = 0.0;      // (the words too: all-zero bits)
  for (int k = 0; k < 12; ++k) { state[kGicpX + k] = x.v[k]; state[kGicpXc + k] = x.v[k]; }
  state[kGicpLambda] = 1e-3;
}

// G3: the side's term (1 - eps) n^ n^T, taken off M = 2 I; a normal that is not finite or has no length leaves the side at I
__device__ __forceinline__ void gicp_side(const float4 n4, double k, double &a, double &b, double &c, double &d, double &e, double &f)
{
  const double x = n4.x, y = n4.y, z = n4.z;
  const double l2 = (x * x + y * y) + z * z;
  if (!(isfinite(x) && isfinite(y) && isfinite(z) && l2 > 0.0)) return;
  const double inv = 1.0 / sqrt(l2);
  const double ux = x * inv, uy = y * inv, uz = z * inv;
  a -= k * (ux * ux); b -= k * (ux * uy); c -= k * (ux * uz);
  d -= k * (uy * uy); e -= k * (uy * uz); f -= k * (uz * uz);
}

// G5.  acc: 0..20 upper triangle of H = sum J^T W J (row-major), 21..26 g = sum J^T W r, 27 count, 28 f = sum r^T W r
__global__ void __launch_bounds__(kRT)
gicp_sums_kernel(const float4 *__restrict__ src, const float4 *__restrict__ snrm, const float4 *__restrict__ tgt,
                 const float4 *__restrict__ tnrm, const int32_t *__restrict__ match, const uint32_t *__restrict__ qperm, size_t q_begin,
                 size_t q_count, double eps, double *state, double *__restrict__ partials)
{
  if (gicp_words(state)[kGicpDone] != 0u) return;                  // the optimisation has ended: nothing is read or written
  double X[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) X[k] = state[kGicpXc + k];
  const double kk = 1.0 - eps;
  double acc[29];
#pragma unroll
  for (int k = 0; k < 29; ++k) acc[k] = 0.0;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < q_count; k += stride) {
    const size_t i = qperm ? (size_t)qperm[q_begin + k] : (q_begin + k);
    const int32_t j = match[i];
    if (j < 0) continue;
    const float4 p = src[i], s4 = snrm[i], q = tgt[j], n4 = tnrm[j];
    // G3, G4: M = A + B, W = M^-1 by cofactors (M is symmetric, eigenvalues in [2 eps, 2])
    double a = 2.0, b = 0.0, c = 0.0, d = 2.0, e = 0.0, f = 2.0;
    gicp_side(s4, kk, a, b, c, d, e, f);
    gicp_side(n4, kk, a, b, c, d, e, f);
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
    const double c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
    const double idet = 1.0 / ((a * c00 + b * c01) + c * c02);
    double W[3][3];
    W[0][0] = c00 * idet; W[0][1] = c01 * idet; W[0][2] = c02 * idet;
    W[1][1] = c11 * idet; W[1][2] = c12 * idet; W[2][2] = c22 * idet;
    W[1][0] = W[0][1]; W[2][0] = W[0][2]; W[2][1] = W[1][2];
    const double px = p.x, py = p.y, pz = p.z;
    const double yx = ((X[0] * px + X[1] * py) + X[2] * pz) + X[9];
    const double yy = ((X[3] * px + X[4] * py) + X[5] * pz) + X[10];
    const double yz = ((X[6] * px + X[7] * py) + X[8] * pz) + X[11];
    const double r[3] = {yx - (double)q.x, yy - (double)q.y, yz - (double)q.z};
    // J = [-[y]x | I]: its columns, then W J and W r
    const double J[6][3] = {{0.0, -yz, yy}, {yz, 0.0, -yx}, {-yy, yx, 0.0}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    double WJ[6][3], Wr[3];
#pragma unroll
    for (int cc = 0; cc < 6; ++cc)
#pragma unroll
      for (int rr = 0; rr < 3; ++rr) WJ[cc][rr] = (W[rr][0] * J[cc][0] + W[rr][1] * J[cc][1]) + W[rr][2] * J[cc][2];
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) Wr[rr] = (W[rr][0] * r[0] + W[rr][1] * r[1]) + W[rr][2] * r[2];
    int t = 0;
#pragma unroll
    for (int rr = 0; rr < 6; ++rr)
#pragma unroll
      for (int cc = rr; cc < 6; ++cc) acc[t++] += (J[rr][0] * WJ[cc][0] + J[rr][1] * WJ[cc][1]) + J[rr][2] * WJ[cc][2];
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) acc[21 + rr] += (J[rr][0] * Wr[0] + J[rr][1] * Wr[1]) + J[rr][2] * Wr[2];
    acc[27] += 1.0;
    acc[28] += (r[0] * Wr[0] + r[1] * Wr[1]) + r[2] * Wr[2];
  }
  block_partials<29>(acc, partials);
}

// G6: (H + lambda diag(H)) delta = -g by Cholesky; false for a pivot that is not a positive finite number
__device__ bool gicp_solve6(const double *s, double lambda, double *delta)
{
  double A[6][6], L[6][6], z[6];
  int t = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) { A[r][c] = s[t]; A[c][r] = s[t]; ++t; }
  for (int r = 0; r < 6; ++r) A[r][r] = A[r][r] + lambda * A[r][r];
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0) || !isfinite(d)) return false;
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  for (int i = 0; i < 6; ++i) {
    double v = -s[21 + i];
    for (int k = 0; k < i; ++k) v -= L[i][k] * z[k];
    z[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = z[i];
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * delta[k];
    delta[i] = v / L[i][i];
  }
  return true;
}

// G6: the candidate R_c = E R, t_c = E t + v, E the Rodrigues matrix of omega
__device__ void gicp_candidate(const double *X, const double *delta, double *Xc)
{
  const double wx = delta[0], wy = delta[1], wz = delta[2];
  const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
  double ca, cb;
  if (th < 1e-8) { ca = 1.0; cb = 0.5; }
  else { ca = sin(th) / th; cb = (1.0 - cos(th)) / th2; }
  const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
  double E[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double k2 = (K[r][0] * K[0][c] + K[r][1] * K[1][c]) + K[r][2] * K[2][c];
      E[r][c] = ((r == c ? 1.0 : 0.0) + ca * K[r][c]) + cb * k2;
    }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Xc[3 * r + c] = (E[r][0] * X[c] + E[r][1] * X[3 + c]) + E[r][2] * X[6 + c];
    Xc[9 + r] = ((E[r][0] * X[9] + E[r][1] * X[10]) + E[r][2] * X[11]) + delta[3 + r];
  }
}

// G7, one turn: the sums of the evaluation just made -> accept / reject -> the next candidate, or `done`
__global__ void __launch_bounds__(kRT) gicp_step_kernel(const double *__restrict__ partials, int rows, double *state, GicpOpt o)
{
  uint32_t *w = gicp_words(state);
  if (w[kGicpDone] != 0u) return;                                  // (uniform: the word is written only behind the barriers below)
  double s[29];
  sum_rows<29>(partials, rows, s, nullptr);
  if (threadIdx.x != 0) return;
  uint32_t evals = w[kGicpEvals], done = 0u;
  int status = MVR_OK;
  double lambda = state[kGicpLambda];
  if (o.sums_only) {
    for (int k = 0; k < 29; ++k) state[kGicpSums + k] = s[k];
    w[kGicpEvals] = 1u; w[kGicpDone] = 1u;
    return;
  }
  if (evals == 0u) {                                               // the evaluation at X = I
    for (int k = 0; k < 29; ++k) state[kGicpSums + k] = s[k];
    if (s[27] < 3.0) { done = 1u; status = MVR_E_NOCORR; }
    else {
      const double f0 = s[28] / s[27];
      state[kGicpF0] = f0; state[kGicpF1] = f0;
      if (!isfinite(f0)) { done = 1u; status = MVR_E_SINGULAR; }   // G7: a listed point or a W that is not finite
    }
  } else {
    const double f = state[kGicpSums + 28];
    if (s[28] < f) {                                               // accept: strictly below; a NaN fails
      for (int k = 0; k < 29; ++k) state[kGicpSums + k] = s[k];
      for (int k = 0; k < 12; ++k) state[kGicpX + k] = state[kGicpXc + k];
      state[kGicpF1] = s[28] / s[27];
      lambda = fmax(lambda / 10.0, 1e-9);
      w[kGicpAccepted] = w[kGicpAccepted] + 1u;
      if (state[kGicpStepRot] < o.rot_tol && state[kGicpStepTrans] < o.trans_tol) done = 1u;
    } else {
      lambda = 10.0 * lambda;
      if (lambda > 1e9) done = 1u;
    }
  }
  evals += 1u;
  if (!done) {
    if (evals >= (uint32_t)o.max_inner) done = 1u;
    else {
      double cur[29], X[12], Xc[12], delta[6];
      for (int k = 0; k < 29; ++k) cur[k] = state[kGicpSums + k];
      for (int k = 0; k < 12; ++k) X[k] = state[kGicpX + k];
      if (!gicp_solve6(cur, lambda, delta)) { done = 1u; status = MVR_E_SINGULAR; }
      else {
        gicp_candidate(X, delta, Xc);
        for (int k = 0; k < 12; ++k) state[kGicpXc + k] = Xc[k];
        state[kGicpStepRot] = sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]);
        state[kGicpStepTrans] = sqrt((delta[3] * delta[3] + delta[4] * delta[4]) + delta[5] * delta[5]);
      }
    }
  }
  state[kGicpLambda] = lambda;
  w[kGicpEvals] = evals;
  w[kGicpStatus] = (uint32_t)status;
  w[kGicpDone] = done;
}

}  // namespace

int ensure_gicp_state(Ctx *c)
{
  if (!c->gicp_state) {
    MVR_MAY_BLOCK(c, "the GICP state block is not allocated yet");
    MVR_HIP_TRY(c, hipMalloc(&c->gicp_state, kGicpStateBytes));
    MVR_HIP_TRY(c, hipMemsetAsync(c->gicp_state, 0, kGicpStateBytes, c->stream));
  }
  if (!c->gicp_host) MVR_HIP_TRY(c, hipHostMalloc(reinterpret_cast<void **>(&c->gicp_host), kGicpStateBytes, hipHostMallocDefault));
  return ensure(c, c->partials, c->partials_cap, (size_t)kMaxBlocks * 32);
}

int launch_gicp_init(Ctx *c, const double X[16])
{
  GicpX x;
  const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  for (int k = 0; k < 12; ++k) x.v[k] = I[k];
  if (X) {                                                         // column-major 4x4 -> R row-major, t
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) x.v[3 * r + k] = X[r + 4 * k]; x.v[9 + r] = X[r + 12]; }
  }
  hipLaunchKernelGGL(gicp_init_kernel, dim3(1), dim3(64), 0, c->stream, c->gicp_state, x);
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

int launch_gicp_pairs(Ctx *c, const float4 *src, const float4 *snrm, const float4 *tgt, const float4 *tnrm, const int32_t *match,
                      const uint32_t *qperm, size_t q_begin, size_t q_count, const mvr_gicp_params *p, double eps, bool sums_only,
                      int pairs)
{
  const int blocks = reduce_blocks(c, q_count);
  GicpOpt o;
  o.rot_tol = p ? p->inner_rot_tol : 0.0; o.trans_tol = p ? p->inner_trans_tol : 0.0;
  o.max_inner = p ? p->max_inner_iterations : 1; o.sums_only = sums_only ? 1 : 0;
  ProfScope ps(c, MVR_K_REDUCE, 64.0 * (double)q_count * (double)pairs);
  for (int k = 0; k < pairs; ++k) {
    hipLaunchKernelGGL(gicp_sums_kernel, dim3(blocks), dim3(kRT), 0, c->stream, src, snrm, tgt, tnrm, match, qperm, q_begin, q_count,
                       eps, c->gicp_state, c->partials);
    hipLaunchKernelGGL(gicp_step_kernel, dim3(1), dim3(kRT), 0, c->stream, c->partials, blocks, c->gicp_state, o);
  }
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

int read_gicp_state(Ctx *c)
{
  MVR_HIP_TRY(c, hipMemcpyAsync(c->gicp_host, c->gicp_state, kGicpStateBytes, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MVR_OK;
}

// G7 from the host's side: chunks of evaluation + step pairs, one round trip per chunk (the caller may queue further copies
// before the first of them: `ride`), until the state block says `done`
int gicp_optimise(Ctx *c, const float4 *src, const float4 *snrm, const float4 *tgt, const float4 *tnrm, const int32_t *match,
                  const uint32_t *qperm, size_t q_begin, size_t q_count, const mvr_gicp_params *p, int (*ride)(Ctx *))
{
  if (int rc = launch_gicp_init(c, nullptr)) return rc;
  const int chunk = (p->inner_chunk <= 0 || p->inner_chunk > p->max_inner_iterations) ? p->max_inner_iterations : p->inner_chunk;
  int queued = 0;
  for (;;) {
    const int now = std::min(chunk, p->max_inner_iterations - queued);
    if (int rc = launch_gicp_pairs(c, src, snrm, tgt, tnrm, match, qperm, q_begin, q_count, p, p->gicp_epsilon, false, now)) return rc;
    queued += now;
    if (ride) { if (int rc = ride(c)) return rc; ride = nullptr; }
    if (int rc = read_gicp_state(c)) return rc;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(c->gicp_host + kGicpWordsAt);
    if (w[kGicpDone] != 0u) return MVR_OK;
    if (queued >= p->max_inner_iterations) return set_error(c, MVR_E_HIP, "GICP: the optimiser did not end within max_inner_iterations evaluations");
  }
}

}  // namespace mvr
