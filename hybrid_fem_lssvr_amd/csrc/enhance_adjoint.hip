// Adjoint of the element solve: from W and Wbar = dJ/dW the gradients of J with respect to the
// nodal values, the Dirichlet values and every entry of the collocation tables a, da, c, f.  Per element ONE more solve
// with the forward (M-2)x(M-2) SPD matrix and a second sweep over the collocation points (lssvr_enh_adj.hpp); one
// element per lane (enhance_adjoint_impl.hpp), degrees 3 <= M <= 11 here and 12 <= M <= 16 in enhance_adjoint_b.hip.
// The lane kernel writes the pair (gl, gr) of every element; a second small kernel of the same call sums the pairs of
// the two elements at every node in a fixed order.  FP64, -ffp-contract=off, no atomics, no inline assembly.
#include "enhance_adjoint_impl.hpp"

namespace lssvr {

hipError_t enhance_adjoint_b(const EnhAdjArgs& a, hipStream_t s);
bool enhance_adjoint_elements_host_b(const EnhAdjArgs& a);

namespace {

__global__ __launch_bounds__(kBlock) void enhance_adjoint_gather_kernel(EnhAdjArgs p) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i <= p.ne) enh_adj_gather(p, i);
}

hipError_t enhance_adjoint_a(const EnhAdjArgs& a, hipStream_t s) {
  switch (a.M) {
    LSSVR_EA_CASE_DEVICE(3)
    LSSVR_EA_CASE_DEVICE(4)
    LSSVR_EA_CASE_DEVICE(5)
    LSSVR_EA_CASE_DEVICE(6)
    LSSVR_EA_CASE_DEVICE(7)
    LSSVR_EA_CASE_DEVICE(8)
    LSSVR_EA_CASE_DEVICE(9)
    LSSVR_EA_CASE_DEVICE(10)
    LSSVR_EA_CASE_DEVICE(11)
    default:
      return enhance_adjoint_b(a, s);
  }
}

bool enhance_adjoint_elements_host_a(const EnhAdjArgs& a) {
  switch (a.M) {
    LSSVR_EA_CASE_HOST(3)
    LSSVR_EA_CASE_HOST(4)
    LSSVR_EA_CASE_HOST(5)
    LSSVR_EA_CASE_HOST(6)
    LSSVR_EA_CASE_HOST(7)
    LSSVR_EA_CASE_HOST(8)
    LSSVR_EA_CASE_HOST(9)
    LSSVR_EA_CASE_HOST(10)
    LSSVR_EA_CASE_HOST(11)
    default:
      return enhance_adjoint_elements_host_b(a);
  }
}

}  // namespace

hipError_t enhance_adjoint(const EnhAdjArgs& a, hipStream_t s) {
  const hipError_t rc = enhance_adjoint_a(a, s);
  if (rc != hipSuccess || (!a.gu && !a.gbc)) return rc;
  hipLaunchKernelGGL(enhance_adjoint_gather_kernel, dim3((unsigned)((a.ne + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     s, a);
  return hipGetLastError();
}

bool enhance_adjoint_host(const EnhAdjArgs& a) {
  if (!enhance_adjoint_elements_host_a(a)) return false;
  if (a.gu || a.gbc)
    for (int64_t i = 0; i <= a.ne; ++i) enh_adj_gather(a, i);
  return true;
}

}  // namespace lssvr
