// One (compute, input, output) type combination of the implicit-GEMM conv kernel (see conv_igemm_impl.h);
// split per combination so the ~20 tile/BK/buffering instantiations of each compile in parallel.
#include "conv_igemm_impl.h"

hipError_t launch_conv_bf16_ff(const convimpl::ConvP& p, const convimpl::ConvChoice& c, hipStream_t s) {
    return convimpl::launch_types<__bf16, float, float>(p, c, s);
}
