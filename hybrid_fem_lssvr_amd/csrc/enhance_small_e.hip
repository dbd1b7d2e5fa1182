// Lane-per-element kernels with reaction rows, -(a u')' + c u = f, M = 2 .. kReactSmallMaxM = 16 (see
// enhance_small_impl.hpp).  From M = 17 the fully unrolled body no longer fits 512 registers (124 B of scratch per
// lane at M = 17, 1.1 KB at M = 22): those degrees go to enhance_large_react, which has none.
#include "enhance_small_impl.hpp"

namespace lssvr {
#define LSSVR_RANGE_E(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
static_assert(kReactSmallMaxM == 16, "LSSVR_RANGE_E instantiates M = 2 .. kReactSmallMaxM");
hipError_t enhance_small_react(const EnhanceReactArgs& a, hipStream_t s, const LaunchOpts* o) {
  switch (a.M) {
    LSSVR_RANGE_E(LSSVR_SMALL_CASE_REACT)
    default:
      return hipErrorInvalidValue;
  }
}
}  // namespace lssvr
