// The device side of lssvr_enhance_adjoint: ONE ELEMENT PER LANE, the (M-2)x(M-2) system in
// registers, as in the forward lane kernel (enhance_small_impl.hpp); the arithmetic is enh_adj_element of
// lssvr_enh_adj.hpp, shared with the host mirror.  What this file adds is how a wave reaches memory.
//
// The tables are element-major: a lane walking its own row touches 64 cache lines per instruction.  So the wave loads
// kEaStageK points of its 64 rows at a time with consecutive lanes on consecutive doubles into a wave-private LDS area
// (row pitch kEaStageK + 1: conflict-free when every lane then reads its own row), the way the forward kernel stages
// its tabulated inputs -- and the table rows it computes go back the same way: each lane overwrites the input slot of
// the point it has just consumed (gf over f, ga over a, gda over da, gc over c: an output table always has its input
// table), and after the round's last point the wave stores the area with the same coalesced mapping.  The 64 x M tiles
// of W and Wbar pass through the same area between the two sweeps.  Wave-private LDS: wave barriers only.
#pragma once
#include "lssvr_enh_adj.hpp"

namespace lssvr {

struct EaWaveIO {
  const EnhAdjArgs& p;
  double* stg;          // this wave's area: kEaTilePerWave doubles
  int64_t e0;           // first element of the wave
  int lane;

  __device__ __forceinline__ static void sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ void stage_in(int k0, bool with_f) {
    sync();
#pragma unroll
    for (int i = 0; i < kEaStageK; ++i) {
      const int idx = i * 64 + lane;
      const int row = idx / kEaStageK, kk = idx % kEaStageK;
      const int64_t er = e0 + row;
      const bool in = (er < p.ne) && (k0 + kk < p.n);
      const int64_t g = in ? er * p.n + (k0 + kk) : 0;
      const int o = row * (kEaStageK + 1) + kk;
      if (with_f) stg[o] = in ? p.rhs_values[g] : 0.0;
      if (p.a_values) stg[kEaStageArr + o] = in ? p.a_values[g] : 0.0;
      if (p.da_values) stg[2 * kEaStageArr + o] = in ? p.da_values[g] : 0.0;
      if (p.c_values) stg[3 * kEaStageArr + o] = in ? p.c_values[g] : 0.0;
    }
    sync();
  }
  __device__ __forceinline__ void in(int k, bool with_f, double& f, double& a, double& da, double& c) const {
    const int o = lane * (kEaStageK + 1) + (k & (kEaStageK - 1));
    f = with_f ? stg[o] : 0.0;
    a = p.a_values ? stg[kEaStageArr + o] : 1.0;
    da = p.da_values ? stg[2 * kEaStageArr + o] : 0.0;
    c = p.c_values ? stg[3 * kEaStageArr + o] : 0.0;
  }
  __device__ __forceinline__ void out(int k, double ga, double gda, double gc, double gf) const {
    const int o = lane * (kEaStageK + 1) + (k & (kEaStageK - 1));
    if (p.gf) stg[o] = gf;
    if (p.ga) stg[kEaStageArr + o] = ga;
    if (p.gda) stg[2 * kEaStageArr + o] = gda;
    if (p.gc) stg[3 * kEaStageArr + o] = gc;
  }
  __device__ __forceinline__ void stage_out(int k0) {
    sync();
#pragma unroll
    for (int i = 0; i < kEaStageK; ++i) {
      const int idx = i * 64 + lane;
      const int row = idx / kEaStageK, kk = idx % kEaStageK;
      const int64_t er = e0 + row;
      if ((er < p.ne) && (k0 + kk < p.n)) {
        const int64_t g = er * p.n + (k0 + kk);
        const int o = row * (kEaStageK + 1) + kk;
        // write-once outputs: non-temporal stores, as the forward kernel's W
        if (p.gf) __builtin_nontemporal_store(stg[o], &p.gf[g]);
        if (p.ga) __builtin_nontemporal_store(stg[kEaStageArr + o], &p.ga[g]);
        if (p.gda) __builtin_nontemporal_store(stg[2 * kEaStageArr + o], &p.gda[g]);
        if (p.gc) __builtin_nontemporal_store(stg[3 * kEaStageArr + o], &p.gc[g]);
      }
    }
    sync();
  }
  template <int M>
  __device__ __forceinline__ void tile_rows(const double* src, double (&r)[M]) {
    const int64_t base = e0 * M, total = p.ne * (int64_t)M;
    sync();
#pragma unroll
    for (int i = 0; i < M; ++i) {
      const int64_t idx = base + (int64_t)i * 64 + lane;
      stg[i * 64 + lane] = idx < total ? src[idx] : 0.0;
    }
    sync();
#pragma unroll
    for (int i = 0; i < M; ++i) r[i] = stg[lane * M + i];
  }
  template <int M>
  __device__ __forceinline__ void rows(double (&w)[M], double (&wb)[M]) {
    tile_rows<M>(p.W, w);
    tile_rows<M>(p.Wbar, wb);
  }
};

template <int M>
__global__ __launch_bounds__(kBlock) void enhance_adjoint_kernel(EnhAdjArgs p) {
  __shared__ double tile[(kBlock / 64) * kEaTilePerWave];
  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * kBlock + (tid & ~63);
  if (e0 >= p.ne) return;                                   // (wave-uniform: a whole wave past the end)
  // lanes past the end of the last wave run on a duplicate of the last element, their stores masked: the tables and
  // rows are loaded cooperatively by the wave
  const int64_t e = e0 + (tid & 63);
  const bool live = e < p.ne;
  EaWaveIO io{p, tile + (tid >> 6) * kEaTilePerWave, e0, tid & 63};
  double gl, gr;
  enh_adj_element<M>(p, live ? e : p.ne - 1, io, gl, gr);
  if (live) {
    p.pairs[2 * e] = gl;
    p.pairs[2 * e + 1] = gr;
  }
}

template <int M>
static hipError_t launch_enhance_adjoint(const EnhAdjArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(enhance_adjoint_kernel<M>, dim3((unsigned)((a.ne + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <int M>
static void enhance_adjoint_elements_host(const EnhAdjArgs& a) {
  for (int64_t e = 0; e < a.ne; ++e) {
    EaHostIO io{a, e};
    enh_adj_element<M>(a, e, io, a.pairs[2 * e], a.pairs[2 * e + 1]);
  }
}

#define LSSVR_EA_CASE_DEVICE(MM) \
  case MM:                       \
    return launch_enhance_adjoint<MM>(a, s);
#define LSSVR_EA_CASE_HOST(MM)              \
  case MM:                                  \
    enhance_adjoint_elements_host<MM>(a);   \
    return true;

}  // namespace lssvr
