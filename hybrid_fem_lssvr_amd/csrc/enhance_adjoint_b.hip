// lssvr_enhance_adjoint, degrees 12 <= M <= 16 (the fully unrolled kernels are large: a translation unit of their own
// keeps the build parallel).  See enhance_adjoint.hip.
#include "enhance_adjoint_impl.hpp"

namespace lssvr {

hipError_t enhance_adjoint_b(const EnhAdjArgs& a, hipStream_t s) {
  switch (a.M) {
    LSSVR_EA_CASE_DEVICE(12)
    LSSVR_EA_CASE_DEVICE(13)
    LSSVR_EA_CASE_DEVICE(14)
    LSSVR_EA_CASE_DEVICE(15)
    LSSVR_EA_CASE_DEVICE(16)
    default:
      return hipErrorInvalidValue;
  }
}

bool enhance_adjoint_elements_host_b(const EnhAdjArgs& a) {
  switch (a.M) {
    LSSVR_EA_CASE_HOST(12)
    LSSVR_EA_CASE_HOST(13)
    LSSVR_EA_CASE_HOST(14)
    LSSVR_EA_CASE_HOST(15)
    LSSVR_EA_CASE_HOST(16)
    default:
      return false;
  }
}

}  // namespace lssvr
