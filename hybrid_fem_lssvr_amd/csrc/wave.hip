// Wave problems  rho u_tt + d u_t - (a u')' + c u = f(x, t)  on the P1 mesh, Newmark (beta, gamma) in displacement form
// with a fixed step dt.  Step n+1 solves
//   A u' = load(t_{n+1}) + M_rho (ut / (beta dt^2)) + M_d ((gamma / (beta dt)) ut - vt),
// A the bands of lssvr_p1_assemble_react with c_quad = c + rho / (beta dt^2) + gamma d / (beta dt), (mdiag, moff) and
// (ddiag, doff) those of the same entry with a_quad = 0 and c_quad = rho, d; the solve is lssvr_tridiag_bc_solve_multi.
// This file adds what goes around it, ONE launch per step:
//   advance   the correctors (v', acc') of the step just solved and the right-hand side of the next step
// The right-hand side of row i needs the NEW state at i-1, i, i+1.  Each thread recomputes its neighbours' correctors in
// registers from the old arrays, through the routine that computes its own, so no thread reads what another writes in
// the same launch and no grid barrier is needed; V_out / Acc_out therefore must not be V / Acc.  One pass over the
// nodes, no reduction, no atomics, no LDS, no scratch; phi is read from device memory, so a time loop issues no copy
// and no synchronisation.  Each value comes from one inline routine that the host mirror (lssvr_wave_advance_host)
// calls too: with -ffp-contract=off the two are bit-equal.
// FP64, -ffp-contract=off.
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"

#define LSSVR_WAVE_HD __host__ __device__ __forceinline__

namespace lssvr {

namespace {

// threads per workgroup (four waves) and the grid cap of the grid-stride loop, as timestep.hip
constexpr int kWaveBlock = 256;
constexpr int kWaveMaxBlocks = 1024;

int64_t wave_blocks(int64_t n) {
  const int64_t b = (n + kWaveBlock - 1) / kWaveBlock;
  return b < 1 ? 1 : (b < kWaveMaxBlocks ? b : kWaveMaxBlocks);
}

struct WaveState {
  double u, v, acc;
};

// The state after the step at entry o = j n + i.  U_new == nullptr: (U, V, Acc) is the state.  Else the correctors:
//   ut   = (U + dt V) + c_u2 Acc            c_u2 = (dt dt) (1/2 - beta)
//   vt   = V + c_v1 Acc                     c_v1 = dt (1 - gamma)
//   acc' = (U_new - ut) c_m                 c_m  = 1 / (beta (dt dt))
//   v'   = vt + c_va acc'                   c_va = gamma dt
LSSVR_WAVE_HD WaveState wave_state(const WaveArgs& a, int64_t o) {
  const double u = a.U[o], v = a.V[o], acc = a.Acc[o];
  if (!a.U_new) return WaveState{u, v, acc};
  const double ut = (u + a.dt * v) + a.c_u2 * acc;
  const double vt = v + a.c_v1 * acc;
  const double un = a.U_new[o];
  const double an = (un - ut) * a.c_m;
  return WaveState{un, vt + a.c_va * an, an};
}

// The predictors of the NEXT step from a state, as the two vectors the bands multiply:
//   ut = (u + dt v) + c_u2 acc;   p = c_m ut;   q = c_d ut - (v + c_v1 acc)      c_d = gamma / (beta dt)
// q is not formed without damping bands.
LSSVR_WAVE_HD void wave_pq(const WaveArgs& a, const WaveState& s, double& p, double& q) {
  const double ut = (s.u + a.dt * s.v) + a.c_u2 * s.acc;
  p = a.c_m * ut;
  q = a.ddiag ? a.c_d * ut - (s.v + a.c_v1 * s.acc) : 0.0;
}

// Row i of case j.  The state of node i is written (U_new given); then, with rhs_out, the order of every sum:
//   m   = (moff[i-1] p[i-1] + mdiag[i] p[i]) + moff[i] p[i+1]      (rows 0 and ne: the term of the missing neighbour is
//   dd  = (doff[i-1] q[i-1] + ddiag[i] q[i]) + doff[i] q[i+1]       left out, not added as 0)
//   s   = m + dd                                                   (no damping bands: s = m)
//   out = ((s + phi[0] loads[0][i]) + phi[1] loads[1][i]) + ...    r ascending
LSSVR_WAVE_HD void wave_row(const WaveArgs& a, int j, int64_t i, double* __restrict__ V_out,
                            double* __restrict__ Acc_out, double* __restrict__ rhs_out) {
  const int64_t n = a.ne + 1, o = (int64_t)j * n + i;
  const WaveState s0 = wave_state(a, o);
  if (a.U_new) {
    V_out[o] = s0.v;
    Acc_out[o] = s0.acc;
  }
  if (!rhs_out) return;
  double p, q, pn, qn;
  wave_pq(a, s0, p, q);
  double m = a.mdiag[i] * p;
  double dd = a.ddiag ? a.ddiag[i] * q : 0.0;
  if (i > 0) {
    wave_pq(a, wave_state(a, o - 1), pn, qn);
    m = a.moff[i - 1] * pn + m;
    if (a.ddiag) dd = a.doff[i - 1] * qn + dd;
  }
  if (i < a.ne) {
    wave_pq(a, wave_state(a, o + 1), pn, qn);
    m = m + a.moff[i] * pn;
    if (a.ddiag) dd = dd + a.doff[i] * qn;
  }
  double s = a.ddiag ? m + dd : m;
  const double* phi = a.phi + (int64_t)j * a.R;
  for (int r = 0; r < a.R; ++r) s = s + phi[r] * a.loads[(int64_t)r * n + i];
  rhs_out[o] = s;
}

__global__ __launch_bounds__(kWaveBlock) void wave_advance_kernel(WaveArgs a, double* __restrict__ V_out,
                                                                   double* __restrict__ Acc_out,
                                                                   double* __restrict__ rhs_out) {
  const int64_t n = a.ne + 1, stride = (int64_t)gridDim.x * kWaveBlock;
  for (int64_t i = (int64_t)blockIdx.x * kWaveBlock + threadIdx.x; i < n; i += stride)
    for (int j = 0; j < a.nc; ++j) wave_row(a, j, i, V_out, Acc_out, rhs_out);
}

}  // namespace

void wave_coefficients(WaveArgs& a, double dt, double beta, double gamma) {
  const double dt2 = dt * dt;
  a.dt = dt;
  a.c_u2 = dt2 * (0.5 - beta);
  a.c_v1 = dt * (1.0 - gamma);
  a.c_m = 1.0 / (beta * dt2);
  a.c_d = gamma / (beta * dt);
  a.c_va = gamma * dt;
}

hipError_t wave_advance(const WaveArgs& a, double* V_out, double* Acc_out, double* rhs_out, hipStream_t s) {
  hipLaunchKernelGGL(wave_advance_kernel, dim3((unsigned)wave_blocks(a.ne + 1)), dim3(kWaveBlock), 0, s, a, V_out,
                     Acc_out, rhs_out);
  return hipGetLastError();
}

void wave_advance_host(const WaveArgs& a, double* V_out, double* Acc_out, double* rhs_out) {
  const int64_t n = a.ne + 1;
  for (int j = 0; j < a.nc; ++j)
    for (int64_t i = 0; i < n; ++i) wave_row(a, j, i, V_out, Acc_out, rhs_out);
}

}  // namespace lssvr
